"""GPU test (-m gpu): contour chains and sub-pixel chain points on the batch axis -- cvs_contour_chains_batch and cvs_chain_refine_batch,
contour_chains_batch / chain_refine_batch / contour_edgels_batch -- against the model of chains_batch_model.py, against the single-image
calls on the same device, and against refine_model.py.  Every comparison is exact: np.array_equal on int32, or on the bits of float32."""
import ctypes as C
import functools
import time

import numpy as np
import pytest
import torch

import chains_batch_model as M
import chains_model as CM
import cvsteer_amd as cv
import refine_model as RM
from cvsteer_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
BASE = (37, 259)   # 37: no multiple of the 32-row tile or link block; 259: across the 256-column link block and two tile columns
_handles = {}


def _handle(shape):
    """a handle whose image size is `shape` (the chain call reads no state: any image will do)"""
    shape = tuple(shape)
    if shape not in _handles:
        _handles[shape] = cv.SteerableFiltersG2(torch.zeros(shape, device=DEV))
    return _handles[shape]


def _np(t):
    return t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _bits(a):
    return np.ascontiguousarray(_np(a), F32).view(np.uint32)


def _equal(got, want, what=""):
    for g, w, name in zip(got, want, ("points", "chains", "ranges")):
        g = _np(g)
        assert g.dtype == np.int32 and g.shape == w.shape, (what, name, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name, int(np.count_nonzero((g != w).any(axis=1))))


@functools.lru_cache(maxsize=None)
def _random_case(rows, cols, n, density):
    rng = np.random.default_rng(1000 * rows + cols + n + int(100 * density))
    block = (rng.random((n, rows, cols)) < density).astype(F32)
    if n >= 4:
        block[n // 2] = 0                                                        # an empty plane in the middle
    block.setflags(write=False)
    return block, M.chains_batch(list(block))


def _ptr(a):
    if a is None:
        return None
    return C.c_void_p(a if isinstance(a, int) else (a.data_ptr() if torch.is_tensor(a) else a.ctypes.data))


def _raw(f, planes, pts, cap_p, tab, cap_c, rng, mem, n=None, counts=True):
    """the C call itself -> (status, n_points, n_chains)"""
    arr = cv.api._planes(planes) if planes is not None else None
    a, b = C.c_int(-1), C.c_int(-1)
    rc = L.lib().cvs_contour_chains_batch(f._h, len(planes) if n is None else n, arr, _ptr(pts), cap_p, _ptr(tab), cap_c, _ptr(rng), mem,
                                          C.byref(a) if counts else None, C.byref(b) if counts else None)
    return rc, a.value, b.value


# ---- shapes and densities against the model ----
@pytest.mark.parametrize("rows,cols,n", [BASE + (5,), (1, 1, 3), (2, 65, 4), (33, 130, 7)])
def test_random_planes_against_the_model(rows, cols, n):
    f = _handle((rows, cols))
    for density in (0.03, 0.1, 0.3, 0.6):
        block, want = _random_case(rows, cols, n, density)
        got = f.contour_chains_batch(torch.from_numpy(np.array(block)).to(DEV))
        assert all(t.is_cuda and t.dtype == torch.int32 for t in got)
        print("chains_batch %d x %d x %d density %.2f: %d chains, %d points" % (rows, cols, n, density, len(want[1]), len(want[0])))
        _equal(got, want, density)


# ---- seams ----
def _seam_planes():
    rows, cols = BASE
    p = np.zeros((5, rows, cols), F32)
    p[0, rows - 1, 100] = 1                                                       # the last row of plane 0 ...
    p[1, 0, 99:102] = 1                                                           # ... and row 0 of plane 1: straight and diagonally below it
    p[1, rows - 2, 50:61] = 1                                                     # a T in the last rows of plane 1: a junction at (55, rows - 2)
    p[1, rows - 1, 55] = 1
    p[2, 0, 50:61] = p[2, 4, 50:61] = 1                                           # right below it, a ring whose top side is row 0 of plane 2
    p[2, 0:5, 50] = p[2, 0:5, 60] = 1
    p[3, 10, cols - 1] = p[3, 11, 0] = 1                                          # neighbours in memory, not in the image
    p[3, rows - 1, cols - 1] = p[4, 0, 0] = 1                                     # ... and the same across a seam
    p[4, rows - 1, :] = 1                                                         # the very last row of the block
    return p


def test_nothing_crosses_a_seam():
    f = _handle(BASE)
    rows, cols = BASE
    planes = _seam_planes()
    want = M.chains_batch(list(planes))
    got = f.contour_chains_batch(torch.from_numpy(planes).to(DEV))
    _equal(got, want, "seams")
    pts, tab, rng = (_np(t) for t in got)
    # plane 0 holds one isolated pixel, plane 1 begins with the bar of three: separate chains of separate planes
    assert tab[0].tolist() == [0, 1, 0, 0] and pts[0].tolist() == [100, rows - 1]
    assert tab[1].tolist() == [1, 3, 0, 1] and pts[1:4].tolist() == [[99, 0], [100, 0], [101, 0]]
    # the ring is ONE closed chain of plane 2 from its own smallest pixel; the T above it is three open chains of plane 1
    ring = tab[tab[:, 3] == 2]
    assert ring.shape[0] == 1 and ring[0, 2] == CM.CLOSED and ring[0, 1] == 2 * 11 + 2 * 3
    assert pts[ring[0, 0]].tolist() == [50, 0] and pts[ring[0, 0] + 1].tolist() == [51, 0]
    t_chains = tab[(tab[:, 3] == 1) & (tab[:, 2] != 0)]
    assert t_chains.shape[0] == 3 and not (t_chains[:, 2] & CM.CLOSED).any()
    # x = cols - 1 and x = 0 of consecutive rows, inside a plane and across a seam: four isolated pixels
    p3 = tab[tab[:, 3] == 3]
    assert p3[:, 1].tolist() == [1, 1, 1] and pts[p3[:, 0]].tolist() == [[cols - 1, 10], [0, 11], [cols - 1, rows - 1]]
    p4 = tab[tab[:, 3] == 4]
    assert p4[0].tolist()[1:] == [1, 0, 4] and pts[p4[0, 0]].tolist() == [0, 0]
    assert p4[1, 1] == cols and pts[-1].tolist() == [cols - 1, rows - 1]
    assert rng[:, 0].tolist() == [0, 1, 5, 6, 9, 11]


def test_full_and_empty_planes_side_by_side():
    f = _handle(BASE)
    planes = np.zeros((5,) + BASE, F32)
    planes[1] = planes[3] = 1
    want = M.chains_batch(list(planes))
    got = f.contour_chains_batch(torch.from_numpy(planes).to(DEV))
    _equal(got, want, "full / empty")
    rng = _np(got[2])
    assert rng[0].tolist() == rng[1].tolist() == [0, 0] and rng[2].tolist() == rng[3].tolist() and rng[4].tolist() == rng[5].tolist()
    assert set(_np(got[1])[:, 3].tolist()) == {1, 3}


def test_all_planes_empty():
    f = _handle(BASE)
    for planes in (torch.zeros((5,) + BASE, device=DEV), np.zeros((5,) + BASE, F32)):
        pts, tab, rng = f.contour_chains_batch(planes)
        assert tuple(pts.shape) == (0, 2) and tuple(tab.shape) == (0, 4) and tuple(rng.shape) == (6, 2) and not _np(rng).any()
    d = torch.zeros((5,) + BASE, device=DEV)
    rng = torch.full((6, 2), -9, dtype=torch.int32, device=DEV)
    assert _raw(f, list(d), None, 0, None, 0, rng, L.MEM_DEVICE) == (0, 0, 0)
    torch.cuda.synchronize()
    assert not rng.cpu().numpy().any()


def test_one_plane_is_contour_chains():
    f = _handle(BASE)
    block, _ = _random_case(BASE[0], BASE[1], 5, 0.3)
    m = torch.from_numpy(np.array(block[1])).to(DEV)
    p1, t1 = f.contour_chains(m)
    pts, tab, rng = f.contour_chains_batch(m[None])
    assert torch.equal(pts, p1) and torch.equal(tab, t1) and not bool(tab[:, 3].any())
    assert rng.cpu().tolist() == [[0, 0], [len(t1), len(p1)]]


# ---- inputs ----
def test_mask_kinds_layouts_and_memory():
    rows, cols = BASE
    f = _handle(BASE)
    rng = np.random.default_rng(3)
    v = (rng.random((6, rows, cols)) < 0.25).astype(F32) * rng.random((6, rows, cols), dtype=F32)
    for bad in (np.nan, -1.0, -0.0, np.inf):
        v.reshape(-1)[rng.integers(0, v.size, 300)] = bad
    want = M.chains_batch(list(v))
    assert len(want[1]) > 500
    b = np.where(CM.foreground(v), rng.integers(1, 256, v.shape), 0).astype(np.uint8)
    d, db = torch.from_numpy(v).to(DEV), torch.from_numpy(b).to(DEV)
    _equal(f.contour_chains_batch(d), want, "f32 [N, H, W]")
    _equal(f.contour_chains_batch(d.reshape(2, 3, rows, cols)), want, "f32 [F, K, H, W]")
    _equal(f.contour_chains_batch(db), want, "u8 [N, H, W]")
    _equal(f.contour_chains_batch(db.reshape(3, 2, rows, cols)), want, "u8 [F, K, H, W]")
    keep = [torch.empty(17 * (k + 1), device=DEV) for k in range(6)]            # gaps of different sizes between the planes
    apart = [d[k].clone() for k in range(6)]
    _equal(f.contour_chains_batch(apart), want, "separately allocated planes")
    mixed = [apart[k] if k % 2 else db[k].clone() for k in range(6)]
    _equal(f.contour_chains_batch(mixed), want, "f32 and u8 planes in one call")
    wide = torch.full((6, rows, cols + 9), float("nan"), device=DEV)
    wide[:, :, 3:3 + cols] = d
    _equal(f.contour_chains_batch(wide[:, :, 3:3 + cols]), want, "pitched block")
    _equal(f.contour_chains_batch([wide[k, :, 3:3 + cols] for k in (0, 1, 2, 3, 4, 5)]), want, "pitched views")
    wide_b = torch.full((6, rows, cols + 11), 255, dtype=torch.uint8, device=DEV)
    wide_b[:, :, 2:2 + cols] = db
    _equal(f.contour_chains_batch([wide_b[k, :, 2:2 + cols] for k in range(6)]), want, "pitched u8 views")
    _equal(f.contour_chains_batch([d[k] for k in (0, 0, 0)]), M.chains_batch([v[0]] * 3), "the same plane three times")
    # host planes, host arrays
    got = f.contour_chains_batch(v)
    assert all(isinstance(a, np.ndarray) for a in got)
    _equal(got, want, "f32 host")
    _equal(f.contour_chains_batch(b), want, "u8 host")
    hwide = np.full((6, rows, cols + 4), 1.0, F32)
    hwide[:, :, 2:2 + cols] = v
    _equal(f.contour_chains_batch([hwide[k, :, 2:2 + cols] for k in range(6)]), want, "pitched host views")
    got = f.contour_chains_batch(torch.from_numpy(v))
    assert all(torch.is_tensor(a) and not a.is_cuda for a in got)
    _equal(got, want, "torch CPU")
    # device planes with host arrays, host planes with device arrays: the two memories are independent
    npts, nch = len(want[0]), len(want[1])
    hp, ht, hr = np.full((npts, 2), -9, np.int32), np.full((nch, 4), -9, np.int32), np.full((7, 2), -9, np.int32)
    assert _raw(f, list(d), hp, npts, ht, nch, hr, L.MEM_HOST) == (0, npts, nch)
    _equal((hp, ht, hr), want, "device planes, host arrays")
    dp, dt, dr = (torch.full(a.shape, -9, dtype=torch.int32, device=DEV) for a in (hp, ht, hr))
    assert _raw(f, list(v), dp, npts, dt, nch, dr, L.MEM_DEVICE) == (0, npts, nch)
    _equal((dp, dt, dr), want, "host planes, device arrays")
    del keep


# ---- capacity and identity ----
def test_capacity_and_run_to_run_identity():
    f = _handle(BASE)
    block, want = _random_case(BASE[0], BASE[1], 5, 0.3)
    d = torch.from_numpy(np.array(block)).to(DEV)
    planes = list(d)
    npts, nch = len(want[0]), len(want[1])
    assert _raw(f, planes, None, 0, None, 0, None, L.MEM_DEVICE) == (L.E_SIZE, npts, nch)          # the sizing call
    for mem in (L.MEM_DEVICE, L.MEM_HOST):
        if mem == L.MEM_DEVICE:
            pts, tab, rng = (torch.full(s, -9, dtype=torch.int32, device=DEV) for s in ((npts + 1, 2), (nch + 1, 4), (7, 2)))
        else:
            pts, tab, rng = (np.full(s, -9, np.int32) for s in ((npts + 1, 2), (nch + 1, 4), (7, 2)))
        untouched = lambda: all((_np(a) == -9).all() for a in (pts, tab, rng))
        assert _raw(f, planes, pts, 0, tab, 0, rng, mem) == (L.E_SIZE, npts, nch)                   # sizing with arrays: nothing written
        for cap_p, cap_c in ((npts - 1, nch), (npts, nch - 1)):
            assert _raw(f, planes, pts, cap_p, tab, cap_c, rng, mem) == (L.E_SIZE, npts, nch)
            torch.cuda.synchronize()
            assert untouched()
        assert _raw(f, planes, pts, npts, tab, nch, rng, mem) == (0, npts, nch)
        torch.cuda.synchronize()
        _equal((pts[:npts], tab[:nch], rng[:6]), want, mem)
        assert (_np(pts[npts:]) == -9).all() and (_np(tab[nch:]) == -9).all() and (_np(rng[6:]) == -9).all()   # nothing beyond the counts
    a, b = f.contour_chains_batch(d), f.contour_chains_batch(d)
    assert all(_np(x).tobytes() == _np(y).tobytes() == w.tobytes() for x, y, w in zip(a, b, want))


# ---- errors ----
def test_errors_leave_everything_untouched():
    rows, cols = BASE
    f = _handle(BASE)
    d = (torch.rand((3, rows, cols), device=DEV) < 0.3).float()
    planes = list(d)
    cap = 4 * 3 * rows * cols
    pts = torch.full((cap, 2), -9, dtype=torch.int32, device=DEV)
    tab = torch.full((cap, 4), -9, dtype=torch.int32, device=DEV)
    rng = torch.full((4, 2), -9, dtype=torch.int32, device=DEV)
    D = L.MEM_DEVICE
    bad = lambda *a, **k: _raw(f, *a, **k)[0]
    assert bad(planes, pts, cap, tab, cap, rng, D, n=0) == L.E_BADARG
    assert bad(planes, pts, cap, tab, cap, rng, D, n=-1) == L.E_BADARG
    assert bad(None, pts, cap, tab, cap, rng, D, n=3) == L.E_BADARG
    assert bad(planes, pts, cap, tab, cap, rng, D, counts=False) == L.E_BADARG
    assert bad(planes[:2] + [torch.rand((rows - 1, cols), device=DEV)], pts, cap, tab, cap, rng, D) == L.E_SIZE     # a plane of another size
    assert bad(planes[:2] + [d[2].cpu().numpy()], pts, cap, tab, cap, rng, D) == L.E_BADARG                         # mixed memory
    assert bad(planes[:2] + [torch.zeros((rows, cols), dtype=torch.int32, device=DEV)], pts, cap, tab, cap, rng, D) == L.E_BADARG
    assert bad(planes, pts, cap, tab, cap, None, D) == L.E_BADARG                                                   # a filling call without ranges
    assert bad(planes, None, 5, tab, cap, rng, D) == L.E_BADARG and bad(planes, pts, cap, None, 5, rng, D) == L.E_BADARG
    assert bad(planes, pts, -1, tab, cap, rng, D) == L.E_BADARG and bad(planes, pts, cap, tab, -1, rng, D) == L.E_BADARG
    assert bad(planes, pts, cap, tab, cap, rng, 7) == L.E_BADARG
    assert bad(planes, pts.data_ptr() + 2, cap - 1, tab, cap, rng, D) == L.E_BADARG                                 # not aligned to 4 bytes
    assert bad(planes, pts, cap, tab, cap, rng.data_ptr() + 1, D) == L.E_BADARG
    assert bad(planes, d[1].data_ptr(), 16, tab, cap, rng, D) == L.E_BADARG                                         # points inside a mask
    assert bad(planes, pts, cap, tab, cap, d[2].data_ptr() + 64, D) == L.E_BADARG                                   # ranges inside a mask
    assert bad(planes, pts, cap, pts.data_ptr() + 32, 8, rng, D) == L.E_BADARG                                      # chains inside points
    fresh = cv.SteerableFiltersG2(None)
    fresh._bind_stream(d)
    assert _raw(fresh, planes, pts, cap, tab, cap, rng, D)[0] == L.E_STATE                                          # no setup
    # capture: refused, and the handle works afterwards
    good = f.contour_chains_batch(d)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    junk = torch.zeros(8, device=DEV)
    with torch.cuda.stream(side):
        f.contour_chains_batch(d)                # the handle moves to the side stream outside the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            junk.fill_(1.0)
            rc = _raw(f, planes, pts, cap, tab, cap, rng, D)
    assert rc == (L.E_UNSUPPORTED, -1, -1)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert bool((pts == -9).all()) and bool((tab == -9).all()) and bool((rng == -9).all())
    again = f.contour_chains_batch(d)
    assert all(torch.equal(x, y) for x, y in zip(again, good))
    _equal(good, M.chains_batch(list(d.cpu().numpy())), "after the capture")


def test_more_than_2_to_28_pixels_is_an_argument_error():
    big = cv.SteerableFiltersG2(torch.zeros((4096, 4096), device=DEV))
    m = torch.ones((4096, 4096), dtype=torch.uint8, device=DEV)
    rng = torch.full((18, 2), -9, dtype=torch.int32, device=DEV)
    # 17 * 2^24 > 2^28: a check of the arguments -- the counts stay as they were, and so does the range table a fitting call would write
    assert _raw(big, [m] * 17, None, 0, None, 0, rng, L.MEM_DEVICE) == (L.E_SIZE, -1, -1)
    torch.cuda.synchronize()
    assert bool((rng == -9).all())
    assert "2^28" in L.lib().cvs_last_error(big._h).decode()
    del big


# ---- end to end ----
@functools.lru_cache(maxsize=None)
def _contours_case():
    """4 frames of 270 x 480 -> (object holding their state, frames, the three un-thinned maps [4, 3, H, W], the 12 masks [12, H, W])"""
    from helpers import rand_image
    frames = torch.stack([torch.from_numpy(rand_image(270, 480, seed=40 + s)) for s in range(4)]).to(DEV)
    f = cv.SteerableFiltersG2(frames[0])
    maps = f.pipeline_batch(frames, outputs=[5, 6, 7])
    hi = float(f.nonmax_batch(maps).max())
    masks = f.contours_batch(frames, 0.05 * hi, 0.2 * hi)
    torch.cuda.synchronize()
    return f, frames, maps, masks.reshape(12, 270, 480), (0.05 * hi, 0.2 * hi)


def test_the_masks_of_contours_batch_end_to_end():
    f, _, _, masks, _ = _contours_case()
    pts, tab, rng = f.contour_chains_batch(masks)
    assert len(tab) > 200 and len(pts) > 2000
    each = [f.contour_chains(masks[z]) for z in range(12)]
    first = np.cumsum([0] + [len(p) for p, _ in each])
    want_t = torch.cat([t for _, t in each]).cpu().numpy().copy()
    want_t[:, 0] += np.repeat(first[:-1], [len(t) for _, t in each])
    want_t[:, 3] = np.repeat(np.arange(12), [len(t) for _, t in each])
    want_r = np.stack([np.cumsum([0] + [len(t) for _, t in each]), first], axis=1).astype(np.int32)
    _equal((pts, tab, rng), (torch.cat([p for p, _ in each]).cpu().numpy(), want_t, want_r), "12 masks")
    # polylines and measures take the concatenated arrays as they are
    vtx, poly, idx = f.chain_polylines(pts, tab, 1.5, return_index=True)
    strength = torch.rand(len(pts), device=DEV)
    got_m = f.chain_measures(pts, tab, strength=strength)
    want_v, want_p, want_i, want_m, v0 = [], [], [], [], 0
    for z, (p, t) in enumerate(each):
        v, pl, ix = f.chain_polylines(p, t, 1.5, return_index=True)
        pl = pl.cpu().numpy().copy()
        pl[:, 0] += v0
        v0 += len(v)
        want_v.append(v.cpu().numpy()), want_p.append(pl), want_i.append(ix.cpu().numpy() + first[z])
        rec = f.chain_measures(p, t, strength=strength[first[z]:first[z + 1]]).copy()
        rec["peak_index"] += np.where(rec["peak_index"] >= 0, first[z], 0).astype(np.int32)
        want_m.append(rec)
    poly = poly.cpu().numpy().copy()
    assert np.array_equal(vtx.cpu().numpy(), np.concatenate(want_v)) and np.array_equal(idx.cpu().numpy(), np.concatenate(want_i))
    want_p = np.concatenate(want_p)
    assert np.array_equal(poly[:, :3], want_p[:, :3])
    assert got_m.tobytes() == np.concatenate(want_m).tobytes()


# ---- chain_refine_batch ----
@functools.lru_cache(maxsize=None)
def _refine_case(shape=(33, 65), frames=2, k=2, zero_theta=False):
    rng = np.random.default_rng(77 + k)
    n = frames * k
    maps = rng.random((frames, k) + shape, dtype=F32)
    theta = np.zeros((frames,) + shape, F32) if zero_theta else (np.pi - 2 * np.pi * rng.random((frames,) + shape)).astype(F32)
    masks = (rng.random((n,) + shape) < 0.2).astype(F32)
    masks[1] = 0                                                                 # a plane without points
    pts, _, ranges = M.chains_batch(list(masks))
    for a in (maps, theta, pts, ranges):
        a.setflags(write=False)
    return maps, theta, pts, ranges


def _up(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def test_refine_theta_zero_is_the_model_bit_for_bit():
    maps, theta, pts, ranges = _refine_case(zero_theta=True)
    f = _handle(maps.shape[2:])
    k = maps.shape[1]
    want = [RM.refine(pts[ranges[z, 1]:ranges[z + 1, 1]], maps[z // k, z % k], theta[z // k]) for z in range(len(ranges) - 1)]
    want_xy, want_st = np.concatenate([w[0] for w in want]), np.concatenate([w[1] for w in want])
    assert len(pts) > 500 and (want_xy != pts).any()
    for path in ("device", "host"):
        if path == "device":
            xy, st = f.chain_refine_batch(_up(pts), _up(ranges), _up(maps), _up(theta))
            assert xy.is_cuda and st.is_cuda
        else:
            xy, st = f.chain_refine_batch(np.array(pts), np.array(ranges), np.array(maps), np.array(theta))
            assert isinstance(xy, np.ndarray) and isinstance(st, np.ndarray)
        assert np.array_equal(_bits(xy), _bits(want_xy)) and np.array_equal(_bits(st), _bits(want_st)), path


def test_refine_random_theta_is_chain_refine_of_each_plane():
    maps, theta, pts, ranges = _refine_case()
    f = _handle(maps.shape[2:])
    frames, k = maps.shape[:2]
    dm, dt, dp, dr = _up(maps), _up(theta), _up(pts), _up(ranges)
    want = [f.chain_refine(dp[ranges[z, 1]:ranges[z + 1, 1]], dm[z // k, z % k], dt[z // k]) for z in range(frames * k)]
    want_xy, want_st = torch.cat([w[0] for w in want]), torch.cat([w[1] for w in want])
    xy, st = f.chain_refine_batch(dp, dr, dm, dt)
    assert np.array_equal(_bits(xy), _bits(want_xy)) and np.array_equal(_bits(st), _bits(want_st))
    # planes at no constant stride take the table: separately allocated maps, pitched theta views
    keep = [torch.empty(13 * (i + 1), device=DEV) for i in range(frames * k)]
    apart = [[dm[i, j].clone() for j in range(k)] for i in range(frames)]
    wide = torch.full((frames, maps.shape[2], maps.shape[3] + 7), float("nan"), device=DEV)
    wide[:, :, 2:2 + maps.shape[3]] = dt
    xy2, st2 = f.chain_refine_batch(dp, dr, apart, [wide[i, :, 2:2 + maps.shape[3]] for i in (0, 1)])
    assert torch.equal(xy2.view(torch.int32), xy.view(torch.int32)) and torch.equal(st2.view(torch.int32), st.view(torch.int32))
    swapped = torch.stack([dt[1], dt[0]])
    xy3, st3 = f.chain_refine_batch(dp, dr, apart, [swapped[1], swapped[0]])                  # theta planes at descending addresses
    assert torch.equal(xy3.view(torch.int32), xy.view(torch.int32)) and torch.equal(st3.view(torch.int32), st.view(torch.int32))
    hxy, hst = f.chain_refine_batch(np.array(pts), np.array(ranges), np.array(maps), np.array(theta))   # one kernel behind both paths
    assert np.array_equal(_bits(hxy), _bits(xy)) and np.array_equal(_bits(hst), _bits(st))
    out = (torch.full_like(xy, -9), torch.full_like(st, -9))
    assert f.chain_refine_batch(dp, dr, dm, dt, out=out)[0] is out[0] and torch.equal(out[0].view(torch.int32), xy.view(torch.int32))
    del keep


def test_refine_own_theta_of_every_frame():
    f, frames, maps, masks, _ = _contours_case()
    pts, tab, rng = f.contour_chains_batch(masks)
    xy, st = f.chain_refine_batch(pts, rng, maps)                                # theta=None: the state of frames 0 .. 3
    r = rng.cpu().numpy()
    for z in range(12):
        f.select_frame(z // 3)
        wxy, wst = f.chain_refine(pts[r[z, 1]:r[z + 1, 1]], maps[z // 3, z % 3])
        assert torch.equal(xy[r[z, 1]:r[z + 1, 1]].view(torch.int32), wxy.view(torch.int32)), z
        assert torch.equal(st[r[z, 1]:r[z + 1, 1]].view(torch.int32), wst.view(torch.int32)), z
    f.select_frame(2)                                                            # the selected frame does not matter
    xy2, st2 = f.chain_refine_batch(pts, rng, maps)
    f.select_frame(0)
    assert torch.equal(xy2.view(torch.int32), xy.view(torch.int32)) and torch.equal(st2.view(torch.int32), st.view(torch.int32))
    assert bool(torch.isfinite(xy).all()) and bool(((xy - pts).abs() <= 0.5).all()) and bool((xy != pts).any())
    # more frames than the handle holds: a state error; a handle without orientation state too
    five = torch.zeros((5, 3, 270, 480), device=DEV)
    with pytest.raises(cv.CvsError) as ei:
        f.chain_refine_batch(pts, torch.zeros((16, 2), dtype=torch.int32, device=DEV), five)
    assert ei.value.status == L.E_STATE
    basis_only = cv.SteerableFiltersG2(torch.zeros((270, 480), device=DEV), setup_flags=cv.api.SETUP_BASIS)
    with pytest.raises(cv.CvsError) as ei:
        basis_only.chain_refine_batch(pts, rng, maps)
    assert ei.value.status == L.E_STATE


def _raw_refine(f, frames, k, maps, theta, pts, n, rng, xy, st, mem):
    pm = cv.api._planes(maps) if maps is not None else None
    pt = cv.api._planes(theta) if theta is not None else None
    return L.lib().cvs_chain_refine_batch(f._h, frames, k, pm, pt, _ptr(pts), n, _ptr(rng), _ptr(xy), _ptr(st), mem)


def test_refine_device_data_is_trusted_for_its_meaning_only():
    maps, theta, pts, ranges = _refine_case()
    f = _handle(maps.shape[2:])
    rows, cols = maps.shape[2:]
    dm, dt = _up(maps), _up(theta)
    flat_m, flat_t = [dm[i, j] for i in range(2) for j in range(2)], list(dt)
    # points one step outside the image: three NaNs, their neighbours in the list untouched
    p = np.array(pts)
    where = (3, 17, 40, 63, 64)
    for i, q in zip(where, ((-1, 0), (cols, 0), (0, rows), (0, -1), (cols, rows))):
        p[i] = q
    good = f.chain_refine_batch(_up(pts), _up(ranges), dm, dt)
    xy, st = f.chain_refine_batch(_up(p), _up(ranges), dm, dt)
    xy, st = _np(xy), _np(st)
    assert np.isnan(xy[list(where)]).all() and np.isnan(st[list(where)]).all()
    rest = np.setdiff1d(np.arange(len(p)), where)
    assert np.array_equal(_bits(xy[rest]), _bits(_np(good[0])[rest])) and np.array_equal(_bits(st[rest]), _bits(_np(good[1])[rest]))
    # a range table full of garbage: the call returns, nothing faults; what it computes is unspecified
    n = len(pts)
    for junk in (np.full((5, 2), -2 ** 31, np.int32), np.full((5, 2), 2 ** 31 - 1, np.int32),
                 np.int32([[9, n], [7, n // 2], [5, -3], [3, 2 * n], [1, 0]]), np.random.default_rng(5).integers(-2 ** 31, 2 ** 31, (5, 2)).astype(np.int32)):
        xy_d, st_d = torch.empty((n, 2), device=DEV), torch.empty((n,), device=DEV)
        assert _raw_refine(f, 2, 2, flat_m, flat_t, _up(pts), n, _up(junk), xy_d, st_d, L.MEM_DEVICE) == 0
        torch.cuda.synchronize()
    # the same on the host is refused before anything is queued
    hxy, hst = np.full((n, 2), -9, F32), np.full((n,), -9, F32)
    hm, ht = [np.array(maps[i, j]) for i in range(2) for j in range(2)], [np.array(t) for t in theta]
    for junk in (np.int32([[0, 0], [1, 5], [2, 4], [3, 6], [4, n]]), np.int32([[0, 1]] + ranges[1:].tolist()), np.int32(ranges[:4].tolist() + [[4, n - 1]])):
        assert _raw_refine(f, 2, 2, hm, ht, np.array(pts), n, junk, hxy, hst, L.MEM_HOST) == L.E_BADARG
    for q in ((cols, 2), (-1, 0), (0, rows), (0, -1)):
        hp = np.array(pts)
        hp[n // 2] = q
        assert _raw_refine(f, 2, 2, hm, ht, hp, n, np.array(ranges), hxy, hst, L.MEM_HOST) == L.E_BADARG
    assert (hxy == -9).all() and (hst == -9).all()
    assert _raw_refine(f, 2, 2, hm, ht, np.array(pts), n, np.array(ranges), hxy, hst, L.MEM_HOST) == 0
    assert np.array_equal(_bits(hxy), _bits(good[0])) and np.array_equal(_bits(hst), _bits(good[1]))


def test_refine_argument_errors():
    maps, theta, pts, ranges = _refine_case()
    f = _handle(maps.shape[2:])
    dm, dt, dp, dr = _up(maps), _up(theta), _up(pts), _up(ranges)
    flat_m, flat_t = [dm[i, j] for i in range(2) for j in range(2)], list(dt)
    n = len(pts)
    xy, st = torch.full((n, 2), -9.0, device=DEV), torch.full((n,), -9.0, device=DEV)
    f._bind_stream(dm)
    D = L.MEM_DEVICE
    call = lambda *a: _raw_refine(f, *a)
    assert call(0, 2, flat_m, flat_t, dp, n, dr, xy, st, D) == L.E_BADARG
    assert call(2, 0, flat_m, flat_t, dp, n, dr, xy, st, D) == L.E_BADARG and call(1, 4, flat_m, flat_t[:1], dp, n, dr, xy, st, D) == L.E_BADARG
    assert call(2, 2, None, flat_t, dp, n, dr, xy, st, D) == L.E_BADARG
    assert call(2, 2, flat_m, flat_t, dp, -1, dr, xy, st, D) == L.E_BADARG
    assert call(2, 2, flat_m, flat_t, None, n, dr, xy, st, D) == L.E_BADARG and call(2, 2, flat_m, flat_t, dp, n, None, xy, st, D) == L.E_BADARG
    assert call(2, 2, flat_m, flat_t, dp, n, dr, None, st, D) == L.E_BADARG and call(2, 2, flat_m, flat_t, dp, n, dr, xy, st, 5) == L.E_BADARG
    assert call(2, 2, flat_m, flat_t, dp, n, dr.data_ptr() + 2, xy, st, D) == L.E_BADARG
    assert call(2, 2, flat_m, flat_t, dp, n, dr, dp, st, D) == L.E_BADARG                      # xy is points
    assert call(2, 2, flat_m, flat_t, dp, n, dr, xy, dr, D) == L.E_BADARG                      # strength over ranges
    assert call(2, 2, flat_m, flat_t, dp, n, dr, xy, dm[1, 1].data_ptr() + 400, D) == L.E_BADARG   # strength inside a map
    assert call(2, 2, flat_m, flat_t, dp, n, dr, dt[1], st, D) == L.E_BADARG                   # xy inside a theta plane
    assert call(2, 2, flat_m[:3] + [dm[1, 1][:, :64]], flat_t, dp, n, dr, xy, st, D) == L.E_SIZE
    assert call(2, 2, flat_m, [dt[0], dt[1][:32]], dp, n, dr, xy, st, D) == L.E_SIZE
    plain = cv.SteerableFiltersG2(None)
    plain._bind_stream(dm)
    assert _raw_refine(plain, 2, 2, flat_m, flat_t, dp, n, dr, xy, st, D) == L.E_STATE
    torch.cuda.synchronize()
    assert bool((xy == -9).all()) and bool((st == -9).all())
    assert call(2, 2, flat_m, flat_t, dp, 0, dr, xy, st, D) == 0 and call(2, 2, flat_m, flat_t, None, 0, None, None, None, D) == 0
    assert call(2, 2, flat_m, flat_t, dp, n, dr, xy, None, D) == 0                             # no strength: fine
    torch.cuda.synchronize()
    assert bool(torch.isfinite(xy).all()) and bool((st == -9).all())


def test_refine_captured_graph_replays_on_new_maps():
    maps, theta, pts, ranges = _refine_case()
    f = _handle(maps.shape[2:])
    dm, dt, dp, dr = _up(maps), _up(theta), _up(pts), _up(ranges)
    xy, st = torch.empty((len(pts), 2), device=DEV), torch.empty((len(pts),), device=DEV)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        f.chain_refine_batch(dp, dr, dm, dt, out=(xy, st))            # the handle moves to the side stream outside the capture
        torch.cuda.synchronize()
        xy.fill_(7.0), st.fill_(7.0)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            f.chain_refine_batch(dp, dr, dm, dt, out=(xy, st))
            hxy = np.full((1, 2), -9, F32)                              # host arrays are refused while capturing
            rc = _raw_refine(f, 2, 2, [dm[i, j] for i in range(2) for j in range(2)], list(dt), np.zeros((1, 2), np.int32), 1,
                             np.int32([[0, 0]] * 4 + [[0, 1]]), hxy, None, L.MEM_HOST)
    assert rc == L.E_UNSUPPORTED and (hxy == -9).all()
    torch.cuda.synchronize()
    assert bool((xy == 7.0).all()) and bool((st == 7.0).all())          # a capture runs nothing
    dm.copy_(torch.rand_like(dm))                                        # new contents behind the same pointers
    dt.copy_(torch.rand_like(dt) * 3 - 1.5)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    want_xy, want_st = f.chain_refine_batch(dp, dr, dm, dt)
    assert torch.equal(xy.view(torch.int32), want_xy.view(torch.int32)) and torch.equal(st.view(torch.int32), want_st.view(torch.int32))
    assert bool((xy != 7.0).any())


# ---- composition, and printed times ----
def test_contour_edgels_batch_is_its_composition():
    f, frames, _, _, (low, high) = _contours_case()
    got = f.contour_edgels_batch(frames, low, high, min_area=3, eps=1.0)
    assert len(got) == 9
    maps = f.pipeline_batch(frames, outputs=[5, 6, 7])
    masks = f.link(f.nonmax_batch(maps).reshape(12, 270, 480), low, high, min_area=3, min_peak=0.0)
    pts, tab, rng = f.contour_chains_batch(masks)
    xy, st = f.chain_refine_batch(pts, rng, maps)
    rec = f.chain_measures(pts, tab, strength=st, xy=xy)
    vtx, poly, idx = f.chain_polylines(pts, tab, 1.0, return_index=True)
    for g, w in zip(got, (pts, tab, rng, xy, st, rec, vtx, poly, idx)):
        assert (g.tobytes() == w.tobytes()) if isinstance(w, np.ndarray) else (g.dtype == w.dtype and _np(g).tobytes() == _np(w).tobytes())
    assert len(tab) > 100 and len(f.contour_edgels_batch(frames, low, high)) == 6
    # the masks of that composition are those of contours_batch with the same thresholds
    assert torch.equal(masks.reshape(4, 3, 270, 480), f.contours_batch(frames, low, high, min_area=3))


def test_batch_times_print():
    """wall clock of one batch call against the loop over the 12 masks, and of the refinement against its loop, printed; no threshold"""
    f, _, maps, masks, _ = _contours_case()
    pts, tab, rng = f.contour_chains_batch(masks)                                # (warm: the scratch has its size)
    [f.contour_chains(masks[z]) for z in range(12)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f.contour_chains_batch(masks)
    torch.cuda.synchronize()
    t_batch = time.perf_counter() - t0
    t0 = time.perf_counter()
    each = [f.contour_chains(masks[z]) for z in range(12)]
    torch.cuda.synchronize()
    t_loop = time.perf_counter() - t0
    f.chain_refine_batch(pts, rng, maps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f.chain_refine_batch(pts, rng, maps)
    torch.cuda.synchronize()
    t_rb = time.perf_counter() - t0
    t0 = time.perf_counter()
    for z in range(12):
        f.select_frame(z // 3)
        f.chain_refine(each[z][0], maps[z // 3, z % 3])
    torch.cuda.synchronize()
    t_rl = time.perf_counter() - t0
    f.select_frame(0)
    print("12 masks of 270 x 480, %d chains, %d points: contour_chains_batch %.3f ms, 12 x contour_chains %.3f ms; chain_refine_batch %.3f ms, "
          "12 x (select_frame + chain_refine) %.3f ms" % (len(tab), len(pts), 1e3 * t_batch, 1e3 * t_loop, 1e3 * t_rb, 1e3 * t_rl))
