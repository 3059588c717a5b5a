"""GPU test (-m gpu): contour thinning -- cvs_nonmax against the numpy model (bit for bit outside a thin band of near-ties that the
kernel's cos / sin polynomial may decide differently), the direction convention on synthetic steps and lines, cvs_hysteresis against a
scipy.ndimage.label model byte for byte, every error case, and the Python / C++ surfaces end to end."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import contour_model as M
import cvsteer_amd as cv
from cvsteer_amd import _lib as L
from helpers import rand_image, smooth_image

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _np(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _check_nms(got, m, theta, exact=False, undecided=1e-3):
    """got against the model: identical at every decided pixel, m or +0.0 elsewhere, fewer than `undecided` of the pixels undecided"""
    got, m, theta = _np(got), np.ascontiguousarray(_np(m), np.float32), _np(theta)
    c, s = M.directions(theta)
    want, vb, vf = M.nonmax_parts(m, c, s)
    gb, wb, mb = got.view(np.uint32), want.view(np.uint32), m.view(np.uint32)
    dec = np.ones(m.shape, bool) if exact else M.decided(m, vb, vf)
    assert np.array_equal(gb[dec], wb[dec]), int(np.count_nonzero(gb[dec] != wb[dec]))
    und = ~dec
    assert ((gb[und] == mb[und]) | (gb[und] == 0)).all()
    assert (gb[np.isnan(m)] == 0).all()   # NaN in m always stores +0.0
    n_und = int(np.count_nonzero(und))
    print("nonmax %s: %d undecided of %d" % (m.shape, n_und, m.size))
    assert n_und < undecided * m.size or n_und == 0


def _g2(img, opts=None):
    f = cv.SteerableFiltersG2(None)
    for o, v in (opts or {}).items():
        f.set_option(o, v)
    f.setup(img)
    return f


def _random_case(rows, cols, seed, sprinkle=True):
    rng = np.random.default_rng(seed)
    maps = [rng.random((rows, cols), dtype=np.float32) * np.float32(4) - np.float32(1) for _ in range(3)]
    th = ((rng.random((rows, cols)) - 0.5) * np.pi).astype(np.float32)
    th.flat[rng.integers(0, th.size, max(1, th.size // 50))] = 0.0
    for v in (np.pi / 4, -np.pi / 4, np.pi / 2):
        th.flat[rng.integers(0, th.size, max(1, th.size // 100))] = np.float32(v)
    if sprinkle and rows * cols >= 4096:
        for m in maps:
            k = max(1, m.size // 100000)
            m.flat[rng.integers(0, m.size, k)] = np.nan
            m.flat[rng.integers(0, m.size, k)] = np.inf
        th.flat[rng.integers(0, th.size, max(1, th.size // 100000))] = np.nan
    return maps, th


@pytest.mark.parametrize("kind", ["g2", "g4"])
def test_fish_through_pipeline(fish, kind):
    img = torch.from_numpy(fish).to(DEV)
    f = cv.SteerableFiltersG2(None) if kind == "g2" else cv.SteerableFiltersG4(None, extensions=True)
    outs = f.pipeline(img)
    maps = outs[5:8]
    thin = f.nonmax(maps)
    th = f.getDominantOrientationAngle()
    for t, m in zip(thin, maps):
        # the fish's flat background gives exact plateaus (equal neighbours), true ties: 60 of 47360 pixels in the first MI355X run
        _check_nms(t, m, th, undecided=2e-3)


@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (29, 1), (2, 2), (3, 257), (1080, 1920), (4096, 4096)])
def test_random_maps(shape):
    maps, th = _random_case(*shape, seed=shape[0] * 7 + shape[1])
    f = _g2(torch.from_numpy(rand_image(*shape)).to(DEV))
    dm = [torch.from_numpy(m).to(DEV) for m in maps]
    dth = torch.from_numpy(th).to(DEV)
    for n in (1, 2, 3):
        got = f.nonmax(dm[:n], theta=dth)
        for g, m in zip(got, maps[:n]):
            _check_nms(g, m, th)
    # theta exactly 0 everywhere: w = 0 on both sides, every pixel bit-identical
    zero = torch.zeros(shape, device=DEV)
    for g, m in zip(f.nonmax(dm, theta=zero), maps):
        _check_nms(g, m, np.zeros(shape, np.float32), exact=True)
    # host planes give the device planes' values
    host = f.nonmax(maps, theta=th)
    dev = f.nonmax(dm, theta=dth)
    for a, b in zip(host, dev):
        assert np.array_equal(a.view(np.uint32), b.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("layout", [0, 1, 2, 3])
def test_pitched_planes_and_state_layouts(layout):
    rows, cols = 150, 203
    img = torch.from_numpy(smooth_image(rows, cols)).to(DEV)
    f = _g2(img, {L.OPT_STATE_LAYOUT: layout})
    maps = f.pipeline(img)[5:8]
    th = f.getDominantOrientationAngle()
    # pitched inputs and outputs: column windows of wider buffers
    wide_in = torch.full((rows, 3 * (cols + 9)), float("nan"), device=DEV)
    ins = [wide_in[:, k * (cols + 9) + 3: k * (cols + 9) + 3 + cols] for k in range(3)]
    for a, b in zip(ins, maps):
        a.copy_(b)
    wide_out = torch.full((rows, 3 * (cols + 5)), float("nan"), device=DEV)
    outs = [wide_out[:, k * (cols + 5) + 1: k * (cols + 5) + 1 + cols] for k in range(3)]
    got = f.nonmax(ins, out=outs)
    ref = f.nonmax(maps)
    for g, r, m in zip(got, ref, maps):
        assert torch.equal(g, r)
        _check_nms(g, m, th)


def test_selected_frame_of_a_batch():
    frames = torch.stack([torch.from_numpy(rand_image(96, 128, seed=s)) for s in range(3)]).to(DEV)
    f = cv.SteerableFiltersG2(frames[0])
    out = f.pipeline_batch(frames)
    f.select_frame(2)
    maps = [out[2, k] for k in (5, 6, 7)]
    got = f.nonmax(maps)
    th = f.getDominantOrientationAngle()
    for g, m in zip(got, maps):
        _check_nms(g, m, th)
    f.select_frame(0)
    assert not all(torch.equal(a, b) for a, b in zip(f.nonmax(maps), got))


def test_non_default_stream():
    img = torch.from_numpy(smooth_image(300, 400)).to(DEV)
    f = _g2(img)
    maps = f.pipeline(img)[5:8]
    want = f.nonmax(maps)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = f.nonmax(maps)
    s.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize("kind", ["step", "line"])
@pytest.mark.parametrize("polarity", [1, -1])
def test_geometry(kind, polarity):
    for deg in M.ANGLES:
        img, d = M.feature_image(64, deg, kind, polarity)
        f = _g2(torch.from_numpy(img).to(DEV))
        maps = f.pipeline(torch.from_numpy(img).to(DEV))[5:8]
        k = int(np.argmax([float(m.max()) for m in maps]))
        thin = f.nonmax(maps[k]).cpu().numpy()
        off, bad, narrow, looked = M.geometry_report(maps[k].cpu().numpy(), thin, d, deg)
        assert looked > 20 and off == 0 and bad == 0 and narrow == 0, (deg, off, bad, narrow, looked)


# ---- hysteresis ----
def _check_hyst(got, v, low, high):
    want = M.hysteresis(_np(v), low, high)
    g = _np(got)
    if g.dtype == np.float32:
        assert set(np.unique(g).tolist()) <= {0.0, 255.0}
        g = g.astype(np.uint8)
    assert np.array_equal(g, want), int(np.count_nonzero(g != want))


@pytest.mark.parametrize("low, high", [(0.5, 0.9), (0.3, 0.95), (0.7, 0.7), (-1.0, 0.99), (2.0, 3.0), (-3.0, -2.0)])
def test_hysteresis_random(low, high):
    rng = np.random.default_rng(int(100 * abs(high)))
    v = rng.random((517, 731), dtype=np.float32)
    v.flat[rng.integers(0, v.size, 50)] = np.nan
    f = _g2(torch.from_numpy(rand_image(517, 731)).to(DEV))
    dv = torch.from_numpy(v).to(DEV)
    for dtype in (torch.uint8, torch.float32):
        _check_hyst(f.hysteresis(dv, low, high, dtype=dtype), v, low, high)
        _check_hyst(f.hysteresis(v, low, high, dtype=dtype), v, low, high)   # host planes


def test_hysteresis_thinned_fish_and_three_at_once(fish):
    img = torch.from_numpy(fish).to(DEV)
    f = cv.SteerableFiltersG2(img)
    thin = f.nonmax(f.pipeline(img)[5:8])
    hi = float(max(float(t.max()) for t in thin))
    low, high = 0.05 * hi, 0.2 * hi
    three, passes = f.hysteresis(list(thin), low, high, return_passes=True)
    assert passes >= 1
    for t, g in zip(thin, three):
        _check_hyst(g, t, low, high)
        assert torch.equal(g, f.hysteresis(t, low, high))


@pytest.mark.parametrize("where, dtype", [("host", np.uint8), ("host", np.float32), ("device-padded", torch.uint8), ("device", torch.float32)])
def test_hysteresis_two_groups_every_output_route(where, dtype):
    """4 planes of 37 x 70: more than the three planes of one group, so the second group reuses the label scratch; 70 columns are no
    multiple of 64, so host bytes are staged at a pitch that is not the row width.  Host bytes, host f32, device bytes with padded rows
    (column slices of a wider tensor, whose padding stays as it was) and device f32."""
    rows, cols, low, high = 37, 70, 0.5, 0.9
    rng = np.random.default_rng(3770)
    vs = [rng.random((rows, cols), dtype=np.float32) for _ in range(4)]
    f = _g2(torch.from_numpy(rand_image(rows, cols)).to(DEV))
    if where == "host":
        got = f.hysteresis(vs, low, high, dtype=dtype)
        assert all(isinstance(g, np.ndarray) and g.dtype == dtype for g in got)
    else:
        dvs = [torch.from_numpy(v).to(DEV) for v in vs]
        wide = torch.full((4, rows, cols + 26), 7, dtype=dtype, device=DEV) if where == "device-padded" else None
        out = None if wide is None else [wide[k, :, :cols] for k in range(4)]
        got = f.hysteresis(dvs, low, high, dtype=dtype, out=out)
        assert all(g.is_cuda and g.dtype == dtype for g in got)
        if wide is not None:
            assert all(g.stride(0) == cols + 26 for g in got) and bool((wide[:, :, cols:] == 7).all())
    assert len(got) == 4
    for g, v in zip(got, vs):
        _check_hyst(g, v, low, high)


def test_hysteresis_serpentine():
    """a 1-pixel path across a 1024 x 1024 image with its only strong pixel at one end"""
    n = 1024
    v = np.zeros((n, n), np.float32)
    for r in range(1, n - 1, 4):
        v[r, 1:n - 1] = 0.5
        turn = n - 2 if (r // 4) % 2 == 0 else 1
        if r + 4 < n - 1:
            v[r + 1:r + 4, turn] = 0.5
    v[1, 1] = 1.0
    f = _g2(torch.from_numpy(rand_image(n, n)).to(DEV))
    got, passes = f.hysteresis(torch.from_numpy(v).to(DEV), 0.25, 0.75, return_passes=True)
    print("serpentine: %d passes" % passes)
    g = got.cpu().numpy()
    assert np.array_equal(g == 255, v > 0) and np.isfinite(passes) and passes > 0


# ---- errors: a code each, and nothing written ----
def test_errors():
    rows, cols = 64, 96
    img = torch.from_numpy(smooth_image(rows, cols)).to(DEV)
    f = _g2(img)
    lib = L.lib()
    ins = [torch.rand(rows, cols, device=DEV) for _ in range(4)]
    outs = [torch.full((rows, cols), 7.0, device=DEV) for _ in range(4)]
    pl = lambda ts: (L.Plane * len(ts))(*[cv.api._plane(t) for t in ts])
    small = torch.rand(rows - 1, cols, device=DEV)
    assert lib.cvs_nonmax(f._h, None, 0, pl(ins[:1]), pl(outs[:1])) == L.E_BADARG
    assert lib.cvs_nonmax(f._h, None, 4, pl(ins), pl(outs)) == L.E_BADARG
    assert lib.cvs_nonmax(f._h, None, 1, pl(ins[:1]), pl(ins[:1])) == L.E_BADARG                  # out is the input
    assert lib.cvs_nonmax(f._h, None, 2, pl(ins[:2]), pl([outs[0], outs[0]])) == L.E_BADARG      # two outputs share memory
    assert lib.cvs_nonmax(f._h, C.byref(cv.api._plane(outs[0])), 1, pl(ins[:1]), pl(outs[:1])) == L.E_BADARG   # out is theta
    assert lib.cvs_nonmax(f._h, None, 1, pl([small]), pl(outs[:1])) == L.E_SIZE
    th_view = L.Plane()
    assert lib.cvs_state_plane(f._h, L.PLANE_THETA, C.byref(th_view)) == 0
    assert lib.cvs_nonmax(f._h, None, 1, pl(ins[:1]), (L.Plane * 1)(th_view)) == L.E_BADARG      # out is the handle's own theta
    fb = cv.SteerableFiltersG2(None)
    fb.setup(img, flags=cv.SETUP_BASIS)
    assert lib.cvs_nonmax(fb._h, None, 1, pl(ins[:1]), pl(outs[:1])) == L.E_STATE
    f4 = cv.SteerableFiltersG4(img)
    assert lib.cvs_nonmax(f4._h, None, 1, pl(ins[:1]), pl(outs[:1])) == L.E_STATE                # G4 without the extension
    with pytest.raises(L.CvsError):
        f4.nonmax(ins[0])
    p = C.c_int(-1)
    assert lib.cvs_hysteresis(f._h, 1, pl(ins[:1]), 0.8, 0.2, pl(outs[:1]), C.byref(p)) == L.E_BADARG
    assert lib.cvs_hysteresis(f._h, 1, pl(ins[:1]), float("nan"), 0.2, pl(outs[:1]), None) == L.E_BADARG
    assert lib.cvs_hysteresis(f._h, 1, pl(ins[:1]), 0.2, float("nan"), pl(outs[:1]), None) == L.E_BADARG
    assert lib.cvs_hysteresis(f._h, 0, pl(ins[:1]), 0.2, 0.8, pl(outs[:1]), None) == L.E_BADARG
    assert lib.cvs_hysteresis(f._h, 1, pl(ins[:1]), 0.2, 0.8, pl(ins[:1]), None) == L.E_BADARG
    assert lib.cvs_hysteresis(f._h, 2, pl(ins[:2]), 0.2, 0.8, pl([outs[1], outs[1]]), None) == L.E_BADARG
    assert lib.cvs_hysteresis(f._h, 1, pl([small]), 0.2, 0.8, pl(outs[:1]), None) == L.E_SIZE
    assert p.value == -1
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == 7.0).all())
    # capture: nonmax is capturable, hysteresis refuses
    maps = f.pipeline(img)[5:8]
    want = f.nonmax(maps)
    got = [torch.empty_like(m) for m in maps]
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        f.nonmax(maps, out=got)                 # the handle moves to the side stream outside the capture
        torch.cuda.synchronize()
        for o in got:
            o.fill_(7.0)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            f.nonmax(maps, out=got)
            rc = lib.cvs_hysteresis(f._h, 1, pl(maps[:1]), 0.2, 0.8, pl(outs[:1]), None)
    assert rc == L.E_UNSUPPORTED
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_contours_end_to_end(fish):
    img = torch.from_numpy(fish).to(DEV)
    f = cv.SteerableFiltersG2(img)
    got = f.contours(img, 20.0, 60.0)
    maps = f.pipeline(img)
    want = f.hysteresis(f.nonmax(maps[5:8]), 20.0, 60.0)
    assert len(got) == 3 and all(g.dtype == torch.uint8 for g in got)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_facade_members(tmp_path, fish):
    exe = os.path.join(str(tmp_path), "test_contours")
    lib = os.path.join(ROOT, "cvsteer_amd")
    if not os.path.exists(os.path.join(lib, "libcvsteer.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cvsteer_amd", "facade"), "-s"])
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-DCVSTEER_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_contours.cpp"), "-L" + lib, "-lcvsteer", "-lcvsteer_hip",
                           "-Wl,-rpath," + lib])
    raw = os.path.join(str(tmp_path), "fish.f32")
    fish.astype(np.float32).tofile(raw)
    r = subprocess.run([exe, raw, str(fish.shape[0]), str(fish.shape[1])], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "contours OK" in r.stdout
