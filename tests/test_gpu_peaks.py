"""GPU test (-m gpu): orientation peaks (cvs_orientation_peaks / orientation_peaks) bit for bit against the float32 model of
tests/peaks_model.py fed by the steering bank of the same handle, on every route, layout, frame and placement the engine distinguishes;
against the float64 model from the engine's own basis planes; and every refusal."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import cvsteer_amd as cv
from cvsteer_amd import _lib as L
import peaks_model as pm
from helpers import EDGE_SHAPES, rand_image

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32 = np.float32
KS, MS = (4, 5, 16, 32), (1, 2, 4)
CANARY_SLOTS = 4
SHAPES = EDGE_SHAPES + [(24, 70), (256, 192)]


def _make(kind, img, opts=None):
    f = (cv.SteerableFiltersG2 if kind == 2 else cv.SteerableFiltersG4)(None)
    for o, v in (opts or {}).items():
        f.set_option(o, v)
    f.setup(img, flags=cv.SETUP_BASIS)   # basis state is all the call needs
    return f


def _energies(f, K):
    """e_k = g_k * g_k + h_k * h_k in numpy float32 from the steering bank of the same handle (merged code) -> [K, H, W]"""
    g, h = f.steer_bank(pm.sample_angles(K))
    g, h = (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in (g, h))
    with np.errstate(invalid="ignore", over="ignore"):
        return (g * g + h * h).astype(F32)


def _np(x):
    return x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _same(got, want, what=""):
    """angles, energies, count: equal bit for bit (the model writes no NaN, so array_equal is exact)"""
    for g, w, name in zip(got, want, ("angles", "energies", "count")):
        g = _np(g)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert np.array_equal(g, w), (what, name, int((g != w).sum()))


def _data_thresholds(e):
    """thresholds from the data: about half of the local maxima lie on each side of min_energy and of the contrast rule; min_ratio
    0.5 cuts between second peaks.  -> (min_energy, min_ratio, min_contrast), and whether each rule has peaks on both sides"""
    with np.errstate(invalid="ignore", divide="ignore"):
        emax, emin = e.max(0), e.min(0)
        local = (e > np.roll(e, 1, 0)) & (e >= np.roll(e, -1, 0))
        if not local.any() or not (emax > 0).any():
            return (0.0, 0.5, 0.5), False
        me = F32(np.median(e[local]))
        r = ((emax - emin) / emax)[(emax > 0) & np.isfinite(emax)]
        mc = F32(min(max(float(np.median(r)), 0.0), 1.0))
        ratio = (e / emax[None])[local & (emax > 0)[None]]
    split = bool((e[local] > me).any() and (e[local] <= me).any() and (r > mc).any() and (r <= mc).any()
                 and (ratio >= 0.5).any() and (ratio < 0.5).any())
    return (float(me), 0.5, float(mc)), split


def _sweep(f, what, ks=KS, ms=MS, need_split=False):
    """the call against the model over K, M and both threshold sets"""
    for K in ks:
        e = _energies(f, K)
        th, split = _data_thresholds(e)
        assert split or not need_split or K < 16, (what, K, th)
        for M in ms:
            for t in ((0.0, 0.0, 0.0), th):
                got = f.orientation_peaks(K, M, *t)
                _same(got, pm.peaks_f32(e, M, *t), (what, K, M, t))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", [2, 4])
def test_bit_for_bit_on_noise(kind, shape):
    img = (pm.smoothed_noise(*shape, seed=3) if min(shape) >= 24 else rand_image(*shape, seed=3) * F32(255)).astype(F32)
    f = _make(kind, torch.from_numpy(img).to(DEV))
    _sweep(f, (kind, shape), need_split=shape[0] * shape[1] >= 1000)


@pytest.mark.parametrize("kind", [2, 4])
def test_ridge_crossing_and_zero_image(kind):
    for name, img in (("ridge", pm.ridge_image([77])), ("crossing", pm.ridge_image([20, 110])), ("zero", np.zeros((49, 49), F32))):
        f = _make(kind, torch.from_numpy(img).to(DEV))
        _sweep(f, (kind, name))
        a, en, c = (_np(x) for x in f.orientation_peaks(16, 4, 0.0, 0.5, 1e-3))
        if name == "zero":
            assert not c.any() and (a == -1).all() and (en == 0).all()
        elif name == "ridge":
            d = abs(float(np.rad2deg(a[0, 24, 24])) - 167.0)
            assert c[24, 24] == 1 and min(d, 180.0 - d) <= pm.RIDGE_BOUND[(kind, 16)]   # phi + 90 degrees
        else:
            assert c[24, 24] == (2 if kind == 4 else 0)             # G4 separates the arms; G2's energy is flat there


@pytest.mark.parametrize("kind", [2, 4])
def test_nan_and_inf_pixels(kind):
    clean = pm.smoothed_noise(70, 96, seed=5)
    bad = clean.copy()
    spots = ((20, 30), (50, 70))
    bad[spots[0]], bad[spots[1]] = np.nan, np.inf
    fc, fb = _make(kind, torch.from_numpy(clean).to(DEV)), _make(kind, torch.from_numpy(bad).to(DEV))
    _sweep(fb, (kind, "nan"), ks=(5, 16), ms=(2, 4))
    want = [_np(x) for x in fc.orientation_peaks(16, 4, 0.0, 0.0, 0.0)]
    got = [_np(x) for x in fb.orientation_peaks(16, 4, 0.0, 0.0, 0.0)]
    w = fb.width
    reach = np.zeros(clean.shape, bool)
    for r, c in spots:
        reach[r - w:r + w + 1, c - w:c + w + 1] = True
    assert not got[2][reach].any() and (got[0][:, reach] == -1).all() and (got[1][:, reach] == 0).all()
    for g, x in zip(got, want):
        assert np.array_equal(g[..., ~reach], x[..., ~reach])


@pytest.mark.parametrize("kind", [2, 4])
def test_float4_and_dword_routes(kind):
    rows, cols, K, M = 64, 48, 16, 4
    img = torch.from_numpy(pm.smoothed_noise(rows, cols, seed=7)).to(DEV)
    f = _make(kind, img)
    want = pm.peaks_f32(_energies(f, K), M)
    _same(f.orientation_peaks(K, M, 0.0, 0.0, 0.0), want, "float4")
    # a row step larger than the width and a base that is not 16-byte aligned: dwords and bytes
    big = torch.full((2, M, rows, cols + 9), 7.0, device=DEV)
    cbig = torch.full((rows, cols + 3), 7, dtype=torch.uint8, device=DEV)
    out = (big[0, :, :, 1:1 + cols], big[1, :, :, 1:1 + cols], cbig[:, 1:1 + cols])
    assert out[0].data_ptr() % 16 == 4 and out[2].data_ptr() % 4 == 1
    _same(f.orientation_peaks(K, M, 0.0, 0.0, 0.0, out=out), want, "dword")
    assert bool((big[..., 0] == 7).all()) and bool((big[..., 1 + cols:] == 7).all()) and bool((cbig[:, 0] == 7).all()) and bool((cbig[:, 1 + cols:] == 7).all())
    # a 47-column view of the image: no float4 anywhere
    fv = _make(kind, img[:, :47])
    _same(fv.orientation_peaks(K, M, 0.0, 0.0, 0.0), pm.peaks_f32(_energies(fv, K), M), "47 columns")


@pytest.mark.parametrize("kind", [2, 4])
def test_state_layouts_are_equal(kind):
    img = torch.from_numpy(pm.smoothed_noise(70, 129, seed=9)).to(DEV)
    ref = None
    for layout in (0, 1, 2, 3):
        f = _make(kind, img, {L.OPT_STATE_LAYOUT: layout})
        got = [_np(x) for x in f.orientation_peaks(16, 4, 0.0, 0.25, 1e-3)]
        if ref is None:
            ref = got
            _same(got, pm.peaks_f32(_energies(f, 16), 4, 0.0, 0.25, 1e-3), layout)
        _same(got, ref, layout)
        f.setup(img, flags=cv.SETUP_FULL if kind == 2 else cv.SETUP_BASIS)   # with orientation state beside the basis planes
        _same(f.orientation_peaks(16, 4, 0.0, 0.25, 1e-3), ref, (layout, "full"))


def test_u8_image_pipeline_state_and_batch_frames():
    u8 = torch.from_numpy(np.clip(pm.smoothed_noise(60, 100, seed=11) + 128, 0, 255).astype(np.uint8)).to(DEV)
    f = _make(2, u8)
    _sweep(f, "u8", ks=(16,), ms=(2,))
    frames = torch.stack([torch.from_numpy(pm.smoothed_noise(60, 100, seed=s)) for s in (12, 13, 14)]).to(DEV)
    f.pipeline(frames[1])                      # the state a pipeline call leaves behind
    fresh = _make(2, frames[1])
    want = [_np(x) for x in fresh.orientation_peaks(16, 4)]
    _same(f.orientation_peaks(16, 4), want, "pipeline")
    f.pipeline_batch(frames)
    for i in (2, 0):
        f.select_frame(i)
        _same(f.orientation_peaks(16, 4), [_np(x) for x in _make(2, frames[i]).orientation_peaks(16, 4)], ("batch frame", i))
    f4 = cv.SteerableFiltersG4(frames[0], extensions=True)
    f4.pipeline_batch(frames)
    f4.select_frame(1)
    _same(f4.orientation_peaks(16, 2), [_np(x) for x in _make(4, frames[1]).orientation_peaks(16, 2)], "G4 batch frame")


@pytest.mark.parametrize("kind", [2, 4])
def test_host_planes_streams_and_capture(kind):
    rows, cols, K, M = 70, 129, 16, 4
    img = pm.smoothed_noise(rows, cols, seed=15)
    f = _make(kind, torch.from_numpy(img).to(DEV))
    want = [_np(x) for x in f.orientation_peaks(K, M)]
    # host planes, with a row step of their own
    ha, he = np.full((M, rows, cols + 5), 7, F32), np.full((M, rows, cols + 5), 7, F32)
    hc = np.full((rows, cols + 2), 7, np.uint8)
    _same(f.orientation_peaks(K, M, out=(ha[:, :, :cols], he[:, :, :cols], hc[:, :cols])), want, "host")
    assert (ha[:, :, cols:] == 7).all() and (hc[:, cols:] == 7).all()
    # a handle set up on a host image returns host planes
    fh = _make(kind, img)
    got = fh.orientation_peaks(K, M)
    assert all(isinstance(x, np.ndarray) for x in got)
    _same(got, want, "host image")
    # separate device allocations that form no run: staged, the same values
    blk = torch.empty(M + 2, rows, cols, device=DEV)
    sep = ([blk[0], blk[1], blk[3], blk[4]], [torch.empty(rows, cols + 1 + s, device=DEV)[:, :cols] for s in range(M)],   # uneven distances; steps that differ
           torch.empty(rows, cols, dtype=torch.uint8, device=DEV))
    got = f.orientation_peaks(K, M, out=sep)
    torch.cuda.synchronize()
    _same((np.stack([_np(x) for x in got[0]]), np.stack([_np(x) for x in got[1]]), got[2]), want, "separate")
    # a non-default stream, then one capture replayed twice
    side = torch.cuda.Stream()
    out = (torch.empty(M, rows, cols, device=DEV), torch.empty(M, rows, cols, device=DEV), torch.empty(rows, cols, dtype=torch.uint8, device=DEV))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        f.orientation_peaks(K, M, out=out)     # the handle moves to the side stream outside the capture
        side.synchronize()
        _same(out, want, "side stream")
        with torch.cuda.graph(graph, stream=side):
            f.orientation_peaks(K, M, out=out)
            rc = L.lib().cvs_orientation_peaks(f._h, C.byref(_cfg(K, M)), cv.api._planes(sep[0]), None, None)   # staged: refused
    assert rc == L.E_UNSUPPORTED
    torch.cuda.synchronize()
    for _ in range(2):
        for o in out:
            o.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        _same(out, want, "replay")


@pytest.mark.parametrize("kind", [2, 4])
def test_output_subsets(kind):
    f = _make(kind, torch.from_numpy(pm.smoothed_noise(33, 65, seed=17)).to(DEV))
    K, M = 16, 2
    full = [_np(x) for x in f.orientation_peaks(K, M)]
    for mask in range(1, 7):
        out = [torch.full((M, 33, 65), 7.0, device=DEV) if mask & 1 else None, torch.full((M, 33, 65), 7.0, device=DEV) if mask & 2 else None,
               torch.full((33, 65), 7, dtype=torch.uint8, device=DEV) if mask & 4 else None]
        got = f.orientation_peaks(K, M, out=tuple(out))
        for i in range(3):
            assert (got[i] is None) == (out[i] is None)
            if got[i] is not None:
                assert np.array_equal(_np(got[i]), full[i]), (mask, i)


@pytest.mark.parametrize("kind", [2, 4])
def test_against_the_float64_model(kind):
    """the engine's own basis planes (read_state) through the float64 formulas and rules: equal counts outside thin pixels, thin pixels
    within the cap, peaks matched as sets within the tolerances the CPU test measured (peaks_model.F64_*_TOL)"""
    f = _make(kind, torch.from_numpy(pm.smoothed_noise(70, 129, seed=19)).to(DEV))
    b = np.stack([_np(f.basis(p)) for p in range(7 if kind == 2 else 11)])
    for K in (8, 16, 32):
        a32, e32, c32 = (_np(x) for x in f.orientation_peaks(K, 4, 0.0, 0.0, 0.0))
        a64, e64, c64, thin = pm.peaks_f64(b, kind, K, 4)
        frac = float(thin.mean())
        assert frac <= pm.THIN_CAP, frac
        assert np.array_equal(c32[~thin], c64[~thin])
        da, de = pm.match_sets(a32, e32, np.where(thin, 0, c32), a64, e64, np.where(thin, 0, c64))
        print("kind %d K %d: thin %.4f, angle %.3g rad, energy %.3g" % (kind, K, frac, da, de))
        assert da <= pm.F64_ANGLE_TOL and de <= pm.F64_ENERGY_TOL


def _cfg(K=16, M=2, me=0.0, mr=0.25, mc=1e-3, size=None):
    return L.PeaksCfg(C.sizeof(L.PeaksCfg) if size is None else size, K, M, me, mr, mc)


def test_refusals_leave_the_outputs_untouched():
    rows, cols, M = 40, 56, 4
    img = torch.from_numpy(pm.smoothed_noise(rows, cols, seed=21)).to(DEV)
    f = _make(2, img)
    f.setup(img, flags=cv.SETUP_FULL)
    lib = L.lib()
    ang = torch.full((CANARY_SLOTS, rows, cols), 7.0, device=DEV)
    en = torch.full((CANARY_SLOTS, rows, cols), 7.0, device=DEV)
    cnt = torch.full((rows, cols), 7, dtype=torch.uint8, device=DEV)
    pa, pe, pc = cv.api._planes(list(ang)), cv.api._planes(list(en)), cv.api._plane(cnt)

    def call(cfg, a=pa, e=pe, c=pc, h=f):
        return lib.cvs_orientation_peaks(h._h, C.byref(cfg) if cfg is not None else None, a, e, C.byref(c) if c is not None else None)

    nan = float("nan")
    bad = [_cfg(K=3), _cfg(K=33), _cfg(M=0), _cfg(M=5), _cfg(me=nan), _cfg(mr=nan), _cfg(mc=nan), _cfg(mr=-0.01), _cfg(mr=1.01),
           _cfg(mc=-0.01), _cfg(mc=1.01), _cfg(size=C.sizeof(L.PeaksCfg) - 4), _cfg(size=0), None]
    for cfg in bad:
        assert call(cfg) == L.E_BADARG, cfg and [getattr(cfg, n) for n, _ in cfg._fields_]
    assert call(_cfg(M=M), None, None, None) == L.E_BADARG                       # all outputs NULL
    # an output aliasing another output: energies = angles; a slot twice; count inside an angle plane
    assert call(_cfg(M=M), pa, pa, pc) == L.E_BADARG
    assert call(_cfg(M=2), cv.api._planes([ang[0], ang[0]]), pe, pc) == L.E_BADARG
    inside = L.Plane(ang[1].data_ptr(), rows, cols, cols, L.MEM_DEVICE | L.DEPTH_U8)
    assert call(_cfg(M=M), pa, pe, inside) == L.E_BADARG
    # an output aliasing a state plane view: a basis plane, and the theta plane
    for which in (L.PLANE_BASIS0 + 3, L.PLANE_THETA):
        v = L.Plane()
        assert lib.cvs_state_plane(f._h, which, C.byref(v)) == 0
        before = _np(f._state(which))
        assert call(_cfg(M=1), (L.Plane * 1)(v), None, None) == L.E_BADARG
        assert np.array_equal(_np(f._state(which)), before)
    # depth: a byte plane as angles, an f32 plane as count
    assert call(_cfg(M=1), (L.Plane * 1)(pc), None, None) == L.E_BADARG
    assert call(_cfg(M=1), None, None, pa[0]) == L.E_BADARG
    # a plane of another size
    small = torch.full((rows - 1, cols), 7.0, device=DEV)
    assert call(_cfg(M=2), cv.api._planes([ang[0], small]), pe, pc) == L.E_SIZE
    small8 = torch.full((rows, cols - 1), 7, dtype=torch.uint8, device=DEV)
    assert call(_cfg(M=2), pa, pe, cv.api._plane(small8)) == L.E_SIZE
    # a handle without basis state: never set up, and state dropped by CVS_OPT_PERSIST_STATE = 0
    fn = cv.SteerableFiltersG2(None)
    assert call(_cfg(), h=fn) == L.E_STATE
    fp = cv.SteerableFiltersG2(None)
    fp.set_persist(False)
    fp.pipeline(img)
    assert call(_cfg(), h=fp) == L.E_STATE
    torch.cuda.synchronize()
    assert bool((ang == 7).all()) and bool((en == 7).all()) and bool((cnt == 7).all()) and bool((small == 7).all()) and bool((small8 == 7).all())
    # the Python surface: an empty request never reaches the library
    with pytest.raises(ValueError):
        f.orientation_peaks(out=(None, None, None))
    with pytest.raises(L.CvsError) as e:
        f.orientation_peaks(n_angles=3)
    assert e.value.status == L.E_BADARG
    # and the handle works afterwards
    _same(f.orientation_peaks(16, M, 0.0, 0.0, 0.0), pm.peaks_f32(_energies(f, 16), M), "afterwards")


def test_facade(tmp_path):
    exe = os.path.join(str(tmp_path), "test_peaks")
    lib = os.path.join(ROOT, "cvsteer_amd")
    if not os.path.exists(os.path.join(lib, "libcvsteer.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cvsteer_amd", "facade"), "-s"])
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-DCVSTEER_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_peaks.cpp"), "-L" + lib, "-lcvsteer", "-lcvsteer_hip",
                           "-Wl,-rpath," + lib])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "peaks OK" in r.stdout
