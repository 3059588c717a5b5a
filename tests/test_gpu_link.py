"""GPU test (-m gpu): the contour chain on the batch axis -- cvs_link against the model of link_model.py and against cvs_hysteresis ->
cvs_contour_prune on the device, cvs_nonmax_batch against cvs_nonmax per frame, cvs_contours_batch against contours() per frame, the
facade's linkContours and the batch driver's --contours.  Every comparison is exact (torch.equal / np.array_equal): there is nothing to
tolerate.  The two timing tests are conditions without margins: the gaps they check are structural."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import cvsteer_amd as cv
import link_model as M
from cvsteer_amd import _lib as L
from helpers import rand_image
from test_gpu_components import SHAPES, TILE_H, TILE_W, double_spiral, serpentine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
INF = float("inf")
# every threshold family of the CPU grid: low < high, low == high, a negative low, (0, 0), high above every finite value, both negative
THRESHOLDS = ((0.2, 0.7), (0.5, 0.5), (-0.3, 0.4), (0.0, 0.0), (0.1, 2.0), (-1.0, -0.5))
PRUNES = ((0, -INF), (3, -INF), (0, 0.6), (5, 0.9), (1000, 0.0), (2, INF))
_handles = {}


def _handle(shape, kind="g2"):
    """a handle whose image size is `shape` (cvs_link reads no state: any image will do)"""
    key = (tuple(shape), kind)
    if key not in _handles:
        f = cv.SteerableFiltersG2(None) if kind == "g2" else cv.SteerableFiltersG4(None, extensions=True)
        f.setup(torch.zeros(tuple(shape), device=DEV))
        _handles[key] = f
    return _handles[key]


def _random_plane(shape, density, seed):
    """values in (0, 1) on a random support, with NaN, negative and infinite pixels sprinkled"""
    rng = np.random.default_rng(seed)
    v = ((rng.random(shape) < density) * rng.random(shape, dtype=np.float32)).astype(np.float32)
    k = max(1, v.size // 50)
    v.flat[rng.integers(0, v.size, k)] = np.nan
    v.flat[rng.integers(0, v.size, k)] = -rng.random(k, dtype=np.float32)
    v.flat[rng.integers(0, v.size, max(1, k // 8))] = np.inf
    return v


def _old_path(f, planes, low, high, min_area, min_peak, dtype=torch.uint8):
    """what cvs_link replaces, on the device: hysteresis, then prune of that mask weighted by the input"""
    masks = f.hysteresis(list(planes), low, high)
    return f.prune(masks, min_area, weight=list(planes), min_peak=min_peak, dtype=dtype, return_kept=True)


def _check(f, v, low, high, min_area=0, min_peak=-INF, model=True, what=""):
    """one plane: link == model, link == hysteresis -> prune on the device, kept equal, and the same again on a second run"""
    v = np.ascontiguousarray(v, np.float32)
    dv = torch.from_numpy(v).to(DEV)
    got, kept = f.link(dv, low, high, min_area, min_peak, return_kept=True)
    assert got.dtype == torch.uint8 and kept.dtype == torch.int32 and kept.is_cuda
    (ref,), (rk,) = _old_path(f, [dv], low, high, min_area, min_peak)
    assert int(kept) == rk, (what, int(kept), rk)
    assert torch.equal(got, ref), (what, int((got != ref).sum()))
    if model:
        want, wk = M.link(v, low, high, min_area, min_peak)
        assert int(kept) == wk and np.array_equal(got.cpu().numpy(), want), (what, int(kept), wk)
    again, kept2 = f.link(dv, low, high, min_area, min_peak, return_kept=True)
    assert torch.equal(again, got) and int(kept2) == int(kept)
    return got, int(kept)


@pytest.mark.parametrize("shape", SHAPES)
def test_link_random(shape):
    f = _handle(shape)
    big = shape[0] * shape[1] > 1 << 20
    for i, density in enumerate((0.3, 0.45) if big else (0.15, 0.45, 0.8)):
        v = _random_plane(shape, density, seed=11 + i)
        for j, (low, high) in enumerate(THRESHOLDS):
            # every threshold family with one prune each on the large planes (the CPU model takes seconds there), the whole grid below
            prunes = (PRUNES[(i + j) % len(PRUNES)],) if big else PRUNES
            for min_area, min_peak in prunes:
                _, kept = _check(f, v, low, high, min_area, min_peak, model=not (shape[0] > 2000 and j > 1),
                                 what="%s d%.2f (%g, %g) area %d peak %g" % (shape, density, low, high, min_area, min_peak))
        print("link %s density %.2f: last kept %d" % (shape, density, kept))


def test_link_structured(fish):
    s = serpentine()
    f = _handle(s.shape)
    got, kept = _check(f, s, 0.25, 0.75, what="serpentine")
    assert kept == 1 and np.array_equal(got.cpu().numpy() == 255, s > 0)
    assert _check(f, s, 0.25, 0.75, min_area=10 ** 7)[1] == 0
    assert _check(f, s, 0.25, 1.0)[1] == 0                       # the one strong pixel is not > 1.0
    sp = double_spiral()
    sp[sp.shape[0] // 2, :] *= 3.0                                 # both arms get a strong pixel where they cross the middle row
    f = _handle(sp.shape)
    assert _check(f, sp, 0.5, 2.0, what="double spiral")[1] == 2
    assert _check(f, np.where(sp > 0, 1.0, 0.0), 0.5, 2.0)[1] == 0
    for shape in ((1, 1), (3, 257), (517, 731), (1080, 1920)):
        f = _handle(shape)
        zeros, kz = _check(f, np.zeros(shape, np.float32), 0.25, 0.75, what="all background")
        assert kz == 0 and not bool(zeros.any())
        ones, ko = _check(f, np.ones(shape, np.float32), 0.25, 0.75, what="all strong")
        assert ko == 1 and bool((ones == 255).all())
        assert _check(f, np.full(shape, np.nan, np.float32), -1.0, -1.0, what="all NaN")[1] == 0
    # the thinned fish maps, three at once, and one by one
    img = torch.from_numpy(fish).to(DEV)
    g = cv.SteerableFiltersG2(img)
    thin = g.nonmax(g.pipeline(img)[5:8])
    hi = float(max(float(t.max()) for t in thin))
    for min_area, min_peak in ((0, -INF), (0, 0.0), (8, 0.0), (2, 0.5 * hi), (30, 0.3 * hi)):
        got, kept = g.link(list(thin), 0.05 * hi, 0.2 * hi, min_area, min_peak, return_kept=True)
        ref, rk = _old_path(g, thin, 0.05 * hi, 0.2 * hi, min_area, min_peak)
        assert kept.tolist() == list(rk) and all(torch.equal(a, b) for a, b in zip(got, ref))
        for a, t, k in zip(got, thin, kept.tolist()):
            want, wk = M.link(t.cpu().numpy(), 0.05 * hi, 0.2 * hi, min_area, min_peak)
            assert k == wk and np.array_equal(a.cpu().numpy(), want)
            assert torch.equal(a, g.link(t, 0.05 * hi, 0.2 * hi, min_area, min_peak))


def test_link_diagonals_through_tile_corners():
    rows, cols = 3 * TILE_H + 5, 3 * TILE_W + 7
    f = _handle((rows, cols))
    for cy in (TILE_H, 2 * TILE_H, 3 * TILE_H):
        for cx in (TILE_W, 2 * TILE_W, 3 * TILE_W):
            for dx, dy in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
                y0, x0 = cy - (1 if dy > 0 else 0), cx - (1 if dx > 0 else 0)
                m = np.zeros((rows, cols), np.float32)
                for t in range(-3, 5):
                    m[y0 + t * dy, x0 + t * dx] = 0.5
                m[y0 - 3 * dy, x0 - 3 * dx] = 1.0   # the strong pixel at one end, on the other side of the corner from most of it
                m[0, 0] = 0.5                       # and a weak pixel nothing links
                got, kept = _check(f, m, 0.25, 0.75)
                assert kept == 1 and int((got == 255).sum()) == 8
    r, c = np.mgrid[0:rows, 0:cols]
    for m in ((r * TILE_W == c * TILE_H), (r % TILE_H == c % TILE_W), ((r + c) % TILE_H == TILE_H - 1), (r - c == 0), (r + c == cols - 1)):
        v = m.astype(np.float32) * 0.5
        v[np.nonzero(m)[0][0], np.nonzero(m)[1][0]] = 1.0
        _check(f, v, 0.25, 0.75, what="diagonal family")


@pytest.mark.parametrize("kind", ["g2", "g4"])
def test_outputs_memory_pitch_and_block(kind):
    rows, cols, n = 150, 203, 5
    f = _handle((rows, cols), kind)
    vs = [_random_plane((rows, cols), 0.45, seed=20 + k) for k in range(n)]
    args = (0.2, 0.7, 3, 0.8)
    want = [M.link(v, *args) for v in vs]
    block = torch.from_numpy(np.stack(vs)).to(DEV)
    # the constant-stride block path, u8 and f32
    got, kept = f.link(block, *args, return_kept=True)
    assert tuple(got.shape) == (n, rows, cols) and got.dtype == torch.uint8 and kept.tolist() == [k for _, k in want]
    assert all(np.array_equal(got[k].cpu().numpy(), want[k][0]) for k in range(n))
    gf = f.link(block, *args, dtype=torch.float32)
    assert gf.dtype == torch.float32 and torch.equal(gf, got.float())
    # a list of separate allocations (the table path) equals the block
    singles = [torch.from_numpy(v).to(DEV) for v in vs]
    pad = [torch.empty(1000 * (k + 1), device=DEV) for k in range(n)]   # (keeps the allocations from lining up)
    outs, kept2 = f.link(singles, *args, return_kept=True)
    assert len(outs) == n and all(torch.equal(outs[k], got[k]) for k in range(n)) and torch.equal(kept2, kept)
    # more planes than one table launch carries, in scattered order
    order = [(7 * k) % n for k in range(37)]
    many = f.link([singles[k] for k in order], *args)
    assert all(torch.equal(many[i], got[k]) for i, k in enumerate(order))
    del pad
    # pitched planes in and out: views into wider buffers, the rest untouched
    wide_in = torch.full((rows, cols + 9), 5.0, device=DEV)
    wide_in[:, 4:4 + cols] = singles[0]
    wide_out = torch.full((rows, cols + 13), 7, dtype=torch.uint8, device=DEV)
    f.link(wide_in[:, 4:4 + cols], *args, out=wide_out[:, 6:6 + cols])
    assert torch.equal(wide_out[:, 6:6 + cols], got[0]) and bool((wide_out[:, :6] == 7).all()) and bool((wide_out[:, 6 + cols:] == 7).all())
    wide_f = torch.full((rows, cols + 3), 7.0, device=DEV)
    f.link(wide_in[:, 4:4 + cols], *args, out=wide_f[:, 1:1 + cols])
    assert torch.equal(wide_f[:, 1:1 + cols], got[0].float()) and bool((wide_f[:, 0] == 7).all())
    # host planes: u8 and f32, one and many (more than one staged chain)
    h1 = f.link(vs[0], *args)
    assert isinstance(h1, np.ndarray) and h1.dtype == np.uint8 and np.array_equal(h1, want[0][0])
    hs, hk = f.link(vs * 4, *args, return_kept=True)
    assert all(np.array_equal(hs[i], want[i % n][0]) for i in range(4 * n)) and hk.tolist() == [k for _, k in want] * 4
    hf = f.link(vs[:2], *args, dtype=np.float32)
    assert hf[1].dtype == np.float32 and np.array_equal(hf[1].astype(np.uint8), want[1][0])
    # a host input into a device output and the other way round
    dmix = torch.empty((rows, cols), dtype=torch.uint8, device=DEV)
    f.link(vs[2], *args, out=dmix)
    hmix = np.empty((rows, cols), np.uint8)
    f.link(singles[2], *args, out=hmix)
    assert np.array_equal(dmix.cpu().numpy(), want[2][0]) and np.array_equal(hmix, want[2][0])


def test_96_planes_of_1080p_in_one_call():
    """32 x 3 planes of 1080p: 199 Mpix, 2.4 GB of scratch at 12 bytes per pixel -- more than the bound, so several chains"""
    rows, cols, n = 1080, 1920, 96
    f = _handle((rows, cols))
    rng = torch.Generator(device=DEV).manual_seed(5)
    block = torch.rand((n, rows, cols), device=DEV, generator=rng)
    block *= (torch.rand((n, rows, cols), device=DEV, generator=rng) < 0.42)
    block[:, ::97, ::89] = float("nan")
    args = (0.3, 0.97, 12, 0.98)
    got, kept = f.link(block, *args, return_kept=True)
    assert tuple(got.shape) == (n, rows, cols)
    for k in range(n):
        one, k1 = f.link(block[k], *args, return_kept=True)
        assert torch.equal(got[k], one) and int(k1) == int(kept[k]), k
    for k in (0, 47, 95):   # and three of them against the old path and the model
        (ref,), (rk,) = _old_path(f, [block[k]], *args)
        want, wk = M.link(block[k].cpu().numpy(), *args)
        assert torch.equal(got[k], ref) and rk == int(kept[k]) == wk and np.array_equal(got[k].cpu().numpy(), want)
    assert int(kept.sum()) > 0 and bool((got == 255).any())
    # the same planes as a list of views in another order: the table path across chains
    order = list(range(n - 1, -1, -1))
    outs = f.link([block[k] for k in order], *args)
    assert all(torch.equal(outs[i], got[k]) for i, k in enumerate(order))


def _frames(n, rows, cols, seed=3):
    return torch.from_numpy(np.stack([rand_image(rows, cols, seed=seed + i) for i in range(n)])).to(DEV)


def _engine(kind):
    return cv.SteerableFiltersG2(None) if kind == "g2" else cv.SteerableFiltersG4(None, extensions=True)


@pytest.mark.parametrize("kind", ["g2", "g4"])
@pytest.mark.parametrize("nf", [1, 5, 32])
def test_nonmax_batch(kind, nf):
    rows, cols = (240, 331) if nf == 32 else (97, 203)
    frames = _frames(nf, rows, cols)
    f = _engine(kind)
    maps = f.pipeline_batch(frames, outputs=(5, 6, 7)).clone()
    # state theta, an [F, K, H, W] block
    got = f.nonmax_batch(maps)
    assert tuple(got.shape) == tuple(maps.shape)
    want = []
    for i in range(nf):
        f.select_frame(i)
        want.append(torch.stack(f.nonmax(list(maps[i]))))
    f.select_frame(0)
    want = torch.stack(want)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    # explicit theta, block and scattered planes, K = 1 and 2
    theta = torch.stack([(f.select_frame(i), f.getDominantOrientationAngle().clone())[1] for i in range(nf)])
    f.select_frame(0)
    assert torch.equal(f.nonmax_batch(maps, theta=theta).view(torch.int32), want.view(torch.int32))
    g2 = f.nonmax_batch(maps[:, :2], theta=theta)
    assert torch.equal(g2.view(torch.int32), want[:, :2].view(torch.int32))
    pads, scattered, thetas = [], [], []
    for i in range(nf):
        pads.append(torch.empty(100 * (i + 1) + 7, device=DEV))
        scattered.append([maps[i, k].clone() for k in range(3)])
        thetas.append(theta[i].clone())
    outs = f.nonmax_batch(scattered, theta=thetas)
    for i in range(nf):
        for k in range(3):
            assert torch.equal(outs[i][k].view(torch.int32), want[i, k].view(torch.int32)), (i, k)
    outs = f.nonmax_batch([fr[:1] for fr in scattered])   # scattered maps, state theta
    assert all(torch.equal(outs[i][0].view(torch.int32), want[i, 0].view(torch.int32)) for i in range(nf))
    # more frames than the handle holds, and no orientation state
    lib = L.lib()
    blk = cv.SteerableFiltersG2._block_planes
    more = torch.zeros((nf + 1, 1, rows, cols), device=DEV)
    keep = torch.full_like(more, 7.0)
    assert lib.cvs_nonmax_batch(f._h, nf + 1, 1, None, blk(more, 2).ctypes.data_as(L._PP), blk(keep, 2).ctypes.data_as(L._PP)) == L.E_STATE
    fresh = _engine(kind)
    fresh.setup(frames[0], flags=cv.SETUP_BASIS)
    assert lib.cvs_nonmax_batch(fresh._h, 1, 1, None, blk(more, 2).ctypes.data_as(L._PP), blk(keep, 2).ctypes.data_as(L._PP)) == L.E_STATE
    torch.cuda.synchronize()
    assert bool((keep == 7.0).all())


CONTOUR_CASES = [("g2", 8, 517, 731, False), ("g4", 8, 517, 731, False), ("g2", 8, 517, 731, True), ("g4", 8, 517, 731, True),
                 ("g2", 32, 1080, 1920, False), ("g4", 32, 1080, 1920, False)]


@pytest.mark.parametrize("kind,nf,rows,cols,u8", CONTOUR_CASES)
def test_contours_batch(kind, nf, rows, cols, u8, fish):
    reps = -(-rows // fish.shape[0]), -(-cols // fish.shape[1])
    base = np.tile(fish, reps)[:rows, :cols].astype(np.float32)
    rng = np.random.default_rng(9)
    frames = np.stack([np.roll(base, (13 * i, 29 * i), (0, 1)) + 6.0 * rng.random((rows, cols), dtype=np.float32) for i in range(nf)])
    frames = torch.from_numpy(np.clip(frames, 0, 255).astype(np.uint8) if u8 else frames.astype(np.float32)).to(DEV)
    f, ref = _engine(kind), _engine(kind)
    thin0 = ref.nonmax(ref.pipeline(frames[0])[5:8])
    hi = float(max(float(t.max()) for t in thin0))
    low, high = 0.05 * hi, 0.2 * hi
    pairs = ((0, 0.0), (8, 0.0), (2, 0.5 * hi), (30, 0.3 * hi))   # those of test_prune_thinned_fish_and_contours
    for j, (min_area, min_peak) in enumerate(pairs if nf <= 8 else pairs[2:3]):
        got = f.contours_batch(frames, low, high, min_area, min_peak)
        assert tuple(got.shape) == (nf, 3, rows, cols) and got.dtype == torch.uint8
        some = 0
        for i in (range(nf) if j == 0 or nf > 8 else (0, nf - 1)):
            want = ref.contours(frames[i], low, high, min_area, min_peak)
            for k in range(3):
                assert torch.equal(got[i, k], want[k]), (i, k, min_area, min_peak, int((got[i, k] != want[k]).sum()))
                some += int((want[k] == 255).sum())
        assert some > 0
    # the state afterwards is that of pipeline_batch: every frame's planes, frame by frame
    g = _engine(kind)
    g.pipeline_batch(frames, outputs=(5,))
    n = C.c_int(0)
    assert L.lib().cvs_num_frames(f._h, C.byref(n)) == 0 and n.value == nf
    for i in (0, nf // 2, nf - 1):
        f.select_frame(i)
        g.select_frame(i)
        assert torch.equal(f.getDominantOrientationAngle().view(torch.int32), g.getDominantOrientationAngle().view(torch.int32))
        assert torch.equal(f.getDominantOrientationStrength().view(torch.int32), g.getDominantOrientationStrength().view(torch.int32))
        assert torch.equal(f.basis(1).view(torch.int32), g.basis(1).view(torch.int32))


def test_contours_batch_lists_host_frames_and_persist():
    rows, cols, nf = 120, 171, 3
    frames = _frames(nf, rows, cols, seed=40)
    f, ref = _engine("g2"), _engine("g2")
    thin0 = ref.nonmax(ref.pipeline(frames[0])[5:8])
    hi = float(max(float(t.max()) for t in thin0))
    want = [ref.contours(frames[i], 0.05 * hi, 0.3 * hi, 4, 0.0) for i in range(nf)]
    got = f.contours_batch([frames[i].clone() for i in range(nf)], 0.05 * hi, 0.3 * hi, 4, 0.0)          # a list of device planes
    host = f.contours_batch(frames.cpu().numpy(), 0.05 * hi, 0.3 * hi, 4, 0.0)                             # host frames
    assert isinstance(host, np.ndarray) and host.dtype == np.uint8
    for i in range(nf):
        for k in range(3):
            assert torch.equal(got[i, k], want[i][k]) and np.array_equal(host[i, k], want[i][k].cpu().numpy())
    one = f.contours_batch(frames[:1], 0.05 * hi, 0.3 * hi, 4, 0.0)                                        # n = 1
    assert all(torch.equal(one[0, k], want[0][k]) for k in range(3))
    f.set_persist(False)
    with pytest.raises(L.CvsError) as e:
        f.contours_batch(frames, 0.05 * hi, 0.3 * hi)
    assert e.value.status == L.E_STATE and "PERSIST" in str(e.value)
    f.set_persist(True)
    again = f.contours_batch(frames, 0.05 * hi, 0.3 * hi, 4, 0.0)
    assert torch.equal(again, got)


def test_capture_one_graph_serves_every_mask():
    n = 1024
    f = _handle((n, n))
    fresh = cv.SteerableFiltersG2(None)
    masks = [serpentine(n), _random_plane((n, n), 0.45, seed=2), np.zeros((n, n), np.float32)]
    thetas = [np.random.default_rng(s).random((n, n), dtype=np.float32) * 3.0 for s in range(3)]
    buf = torch.zeros((2, n, n), device=DEV)        # the input buffers every replay reads
    th = torch.zeros((1, n, n), device=DEV)
    out = torch.zeros((2, n, n), dtype=torch.uint8, device=DEV)
    kept = torch.zeros(2, dtype=torch.int32, device=DEV)
    thin = torch.zeros((1, 2, n, n), device=DEV)
    fresh.setup(buf[0])
    lib = L.lib()
    blk = cv.SteerableFiltersG2._block_planes
    pin, pout = blk(buf, 1), blk(out, 1)

    def run(h):
        rc = lib.cvs_link(h._h, 2, pin.ctypes.data_as(L._PP), 0.25, 0.75, 2, -INF, pout.ctypes.data_as(L._PP), C.c_void_p(kept.data_ptr()))
        h.nonmax_batch(buf.view(1, 2, n, n), theta=th, out=thin)
        return rc

    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        f._bind_stream(buf)
        assert run(f) == 0                          # the eager warm-up call: the scratch has its size, the handle is on the side stream
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            rc = run(f)
    assert rc == 0
    torch.cuda.synchronize()
    for m, t in zip(masks, thetas):
        buf[0].copy_(torch.from_numpy(m))
        buf[1].copy_(torch.from_numpy(m.T.copy()))
        th[0].copy_(torch.from_numpy(t))
        out.fill_(7)
        kept.fill_(-1)
        thin.fill_(7.0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got, gk, gthin = out.clone(), kept.clone(), thin.clone()
        want, wk = f.link(buf, 0.25, 0.75, 2, -INF, return_kept=True)
        assert torch.equal(got, want) and torch.equal(gk, wk)
        assert torch.equal(gthin.view(torch.int32), f.nonmax_batch(buf.view(1, 2, n, n), theta=th).view(torch.int32))
        for k, plane in enumerate((m, m.T)):
            mw, mk = M.link(plane, 0.25, 0.75, 2)
            assert np.array_equal(got[k].cpu().numpy(), mw) and int(gk[k]) == mk
    # a fresh handle whose scratch is too small: the capture is refused, nothing is written, and the handle works afterwards
    out.fill_(7)
    side2 = torch.cuda.Stream()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side2):
        fresh._bind_stream(buf)
        fresh.sync()
        torch.cuda.synchronize()
        with torch.cuda.graph(g2, stream=side2):
            th.fill_(1.0)
            rc = lib.cvs_link(fresh._h, 2, pin.ctypes.data_as(L._PP), 0.25, 0.75, 2, -INF, pout.ctypes.data_as(L._PP), None)
    assert rc == L.E_UNSUPPORTED and b"eagerly" in lib.cvs_last_error(fresh._h)
    torch.cuda.synchronize()
    g2.replay()
    torch.cuda.synchronize()
    assert bool((out == 7).all())
    assert torch.equal(fresh.link(buf, 0.25, 0.75, 2, -INF), f.link(buf, 0.25, 0.75, 2, -INF))


def test_errors():
    rows, cols = 64, 96
    f = _handle((rows, cols))
    lib = L.lib()
    pl = lambda ts: (L.Plane * len(ts))(*[cv.api._plane(t) for t in ts])
    ins = [torch.rand(rows, cols, device=DEV) for _ in range(3)]
    outs = [torch.full((rows, cols), 7, dtype=torch.uint8, device=DEV) for _ in range(3)]
    fout = torch.full((rows, cols), 7.0, device=DEV)
    small = torch.rand(rows - 1, cols, device=DEV)
    small_out = torch.full((rows - 1, cols), 7, dtype=torch.uint8, device=DEV)
    kept = torch.full((3,), -1, dtype=torch.int32, device=DEV)
    kp = C.c_void_p(kept.data_ptr())
    nan = float("nan")
    link = lib.cvs_link
    assert link(f._h, 1, pl(ins[:1]), 0.8, 0.2, 0, 0.0, pl(outs[:1]), kp) == L.E_BADARG              # low > high
    assert link(f._h, 1, pl(ins[:1]), nan, 0.2, 0, 0.0, pl(outs[:1]), kp) == L.E_BADARG
    assert link(f._h, 1, pl(ins[:1]), 0.2, nan, 0, 0.0, pl(outs[:1]), kp) == L.E_BADARG
    assert link(f._h, 1, pl(ins[:1]), 0.2, 0.8, -1, 0.0, pl(outs[:1]), kp) == L.E_BADARG             # min_area < 0
    assert link(f._h, 1, pl(ins[:1]), 0.2, 0.8, 0, nan, pl(outs[:1]), kp) == L.E_BADARG              # NaN min_peak
    assert link(f._h, 0, pl(ins[:1]), 0.2, 0.8, 0, 0.0, pl(outs[:1]), kp) == L.E_BADARG
    assert link(f._h, 1, None, 0.2, 0.8, 0, 0.0, pl(outs[:1]), kp) == L.E_BADARG
    assert link(f._h, 1, pl(ins[:1]), 0.2, 0.8, 0, 0.0, None, kp) == L.E_BADARG
    assert link(f._h, 2, pl(ins[:2]), 0.2, 0.8, 0, 0.0, pl([outs[0], fout]), kp) == L.E_BADARG       # mixed output depth
    assert link(f._h, 1, pl([fout]), 0.2, 0.8, 0, 0.0, pl([fout]), kp) == L.E_BADARG                 # out is the input
    assert link(f._h, 2, pl([ins[0], fout]), 0.2, 0.8, 0, 0.0, pl([fout, ins[2]]), kp) == L.E_BADARG  # out 0 is input 1
    assert link(f._h, 2, pl(ins[:2]), 0.2, 0.8, 0, 0.0, pl([outs[1], outs[1]]), kp) == L.E_BADARG    # outputs overlap
    assert link(f._h, 1, pl(outs[:1]), 0.2, 0.8, 0, 0.0, pl(outs[1:2]), kp) == L.E_BADARG            # u8 input
    assert link(f._h, 1, pl([small]), 0.2, 0.8, 0, 0.0, pl(outs[:1]), kp) == L.E_SIZE
    assert link(f._h, 1, pl(ins[:1]), 0.2, 0.8, 0, 0.0, pl([small_out]), kp) == L.E_SIZE
    fresh = cv.SteerableFiltersG2(None)
    assert link(fresh._h, 1, pl(ins[:1]), 0.2, 0.8, 0, 0.0, pl(outs[:1]), kp) == L.E_STATE           # no image size
    # cvs_contours_batch
    img = torch.rand((2, rows, cols), device=DEV)
    cb = lib.cvs_contours_batch
    three = lambda: pl(outs[:3] + [o.clone() for o in outs[:3]])
    e = cv.SteerableFiltersG2(None)
    assert cb(e._h, pl(list(img)), 2, 0.8, 0.2, 0, 0.0, three()) == L.E_BADARG
    assert cb(e._h, pl(list(img)), 2, 0.2, 0.8, -1, 0.0, three()) == L.E_BADARG
    assert cb(e._h, pl(list(img)), 2, 0.2, 0.8, 0, nan, three()) == L.E_BADARG
    assert cb(e._h, pl(list(img)), 0, 0.2, 0.8, 0, 0.0, three()) == L.E_BADARG
    assert cb(e._h, pl(list(img)), 1, 0.2, 0.8, 0, 0.0, pl([outs[0], outs[0], outs[1]])) == L.E_BADARG
    assert cb(e._h, pl(list(img)), 1, 0.2, 0.8, 0, 0.0, pl([outs[0], fout, outs[1]])) == L.E_BADARG
    assert cb(e._h, pl(list(img)), 1, 0.2, 0.8, 0, 0.0, pl([small_out, outs[0], outs[1]])) == L.E_SIZE
    e4 = cv.SteerableFiltersG4(None)
    assert cb(e4._h, pl(list(img)), 1, 0.2, 0.8, 0, 0.0, pl(outs[:3])) == L.E_UNSUPPORTED             # G4 without the extension
    e.set_persist(False)
    assert cb(e._h, pl(list(img)), 1, 0.2, 0.8, 0, 0.0, pl(outs[:3])) == L.E_STATE
    torch.cuda.synchronize()
    assert bool((kept == -1).all()) and bool((fout == 7.0).all()) and all(bool((o == 7).all()) for o in outs) and bool((small_out == 7).all())


def _median_ms(fn, reps=5):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def test_link_of_the_serpentine_is_faster_than_hysteresis_of_it():
    """medians of five, wall clock around the call and a synchronisation, as test_label_time_does_not_depend_on_the_shape_of_the_contour"""
    v = torch.from_numpy(serpentine()).to(DEV)
    f = _handle((1024, 1024))
    out = torch.empty((1024, 1024), dtype=torch.uint8, device=DEV)
    f.link(v, 0.25, 0.75, out=out)
    ref = f.hysteresis(v, 0.25, 0.75)   # warm both
    assert torch.equal(out, ref)
    a = _median_ms(lambda: f.link(v, 0.25, 0.75, out=out))
    b = _median_ms(lambda: f.hysteresis(v, 0.25, 0.75))
    print("serpentine 1024^2: link %.3f ms, hysteresis %.3f ms, ratio %.1f" % (a, b, b / a))
    assert a < b


def test_contours_batch_is_faster_than_the_per_frame_loop(fish):
    """32 x 1080p: the loop synchronises the stream 64 times and queues more than a thousand launches; the batch call does neither"""
    rows, cols, nf = 1080, 1920, 32
    base = np.tile(fish, (-(-rows // fish.shape[0]), -(-cols // fish.shape[1])))[:rows, :cols].astype(np.float32)
    frames = torch.from_numpy(np.stack([np.roll(base, (7 * i, 11 * i), (0, 1)) for i in range(nf)])).to(DEV)
    f, ref = _engine("g2"), _engine("g2")
    thin0 = ref.nonmax(ref.pipeline(frames[0])[5:8])
    hi = float(max(float(t.max()) for t in thin0))
    low, high = 0.05 * hi, 0.2 * hi
    loop = lambda: [ref.contours(frames[i], low, high, 8, 0.0) for i in range(nf)]
    got, want = f.contours_batch(frames, low, high, 8, 0.0), loop()   # warm both
    assert all(torch.equal(got[i, k], want[i][k]) for i in range(nf) for k in range(3))
    a = _median_ms(lambda: f.contours_batch(frames, low, high, 8, 0.0))
    b = _median_ms(loop)
    print("contours 32 x 1080p: batch %.2f ms, per-frame loop %.2f ms, ratio %.2f" % (a, b, b / a))
    assert a < b


def test_facade_link(tmp_path, fish):
    exe = os.path.join(str(tmp_path), "test_link")
    lib = os.path.join(ROOT, "cvsteer_amd")
    if not os.path.exists(os.path.join(lib, "libcvsteer.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cvsteer_amd", "facade"), "-s"])
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-DCVSTEER_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_link.cpp"), "-L" + lib, "-lcvsteer", "-lcvsteer_hip",
                           "-Wl,-rpath," + lib])
    raw = os.path.join(str(tmp_path), "fish.f32")
    fish.astype(np.float32).tofile(raw)
    r = subprocess.run([exe, raw, str(fish.shape[0]), str(fish.shape[1])], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "link OK" in r.stdout


def test_driver_contours(tmp_path, fish):
    src, dst = os.path.join(str(tmp_path), "in"), os.path.join(str(tmp_path), "out")
    os.makedirs(src)
    frames = [np.roll(fish, (5 * i, 9 * i), (0, 1)).astype(np.float32) for i in range(3)]
    names = []
    for i, a in enumerate(frames):
        names.append(os.path.join(src, "frame%d.npy" % i))
        np.save(names[-1], a)
    lst = os.path.join(src, "list.txt")
    with open(lst, "w") as fh:
        fh.write("\n".join(names) + "\n")
    r = subprocess.run([sys.executable, "-m", "cvsteer_amd.run", "--input", lst, "--output", dst, "--ext", ".npy", "--contours", "20,60,6"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    f = cv.SteerableFiltersG2(None, 4, 0.67)
    for i, a in enumerate(frames):
        want = f.contours(torch.from_numpy(a).to(DEV), 20.0, 60.0, min_area=6)
        for w, suffix in zip(want, ("_edges", "_lines_dark", "_lines_bright")):
            got = np.load(os.path.join(dst, "frame%d%s.npy" % (i, suffix)))
            assert got.dtype == np.uint8 and np.array_equal(got, w.cpu().numpy()), (i, suffix)
            assert set(np.unique(got)) <= {0, 255}


def test_capture_of_scattered_planes_and_cross_frame_overlap():
    """the table path (planes at no common stride: k_link_table launches fill the device table from their arguments) under capture, and
    an output of frame 0 that overlaps the image of frame 1 is refused with nothing written"""
    rows, cols, n = 96, 160, 19
    f = _handle((rows, cols))
    lib = L.lib()
    ins = [torch.zeros((rows, cols), device=DEV) for _ in range(n)]
    pads = [torch.empty(64 * (k + 1) + 3, device=DEV) for k in range(n)]
    outs = [torch.zeros((rows, cols), dtype=torch.uint8, device=DEV) for _ in range(n)]
    order = [(5 * k) % n for k in range(n)]
    pin = (L.Plane * n)(*[cv.api._plane(ins[k]) for k in order])
    pout = (L.Plane * n)(*[cv.api._plane(outs[k]) for k in order])
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        f._bind_stream(ins[0])
        assert lib.cvs_link(f._h, n, pin, 0.2, 0.7, 3, 0.8, pout, None) == 0   # eager warm-up: scratch sized
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            rc = lib.cvs_link(f._h, n, pin, 0.2, 0.7, 3, 0.8, pout, None)
    assert rc == 0
    del pads
    for seed in (1, 2):
        vs = [_random_plane((rows, cols), 0.45, seed=100 * seed + k) for k in range(n)]
        for k in range(n):
            ins[k].copy_(torch.from_numpy(vs[k]))
            outs[k].fill_(7)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for k in range(n):
            assert np.array_equal(outs[k].cpu().numpy(), M.link(vs[k], 0.2, 0.7, 3, 0.8)[0]), (seed, k)
    # cvs_contours_batch: an output of frame 0 lying on the image of frame 1
    e = cv.SteerableFiltersG2(None)
    imgs = torch.rand((2, rows, cols), device=DEV)
    keep = imgs.clone()
    masks = [torch.full((rows, cols), 7.0, device=DEV) for _ in range(5)]
    pl = lambda ts: (L.Plane * len(ts))(*[cv.api._plane(t) for t in ts])
    bad = pl([imgs[1]] + masks)
    assert lib.cvs_contours_batch(e._h, pl(list(imgs)), 2, 0.2, 0.8, 0, 0.0, bad) == L.E_BADARG
    torch.cuda.synchronize()
    assert torch.equal(imgs, keep) and all(bool((m == 7.0).all()) for m in masks)
    with pytest.raises(ValueError):
        e.contours_batch([], 0.2, 0.8)
