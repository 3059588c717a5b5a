"""GPU test (-m gpu): the steering bank (cvs_steer_bank / steer_bank) against cvs_steer_scalar on the same handle, bit for bit, in
every placement, state layout, frame and kind mix the engine distinguishes -- and every error it reports."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import cvsteer_amd as cv
from cvsteer_amd import _lib as L
from helpers import EDGE_SHAPES, rand_image, smooth_image

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMAX = 32   # kBankMax, cvsteer_amd/csrc/cvs_internal.h: angles per launch
DEV = "cuda:0"


def _thetas(n, seed=0):
    return (np.random.default_rng(seed).random(n, dtype=np.float32) - np.float32(0.5)) * np.float32(4 * np.pi)


def _per_angle(f, thetas, kinds):
    """what n separate steer_scalar calls give, kinds picked out of (g, h, e, magnitude, phase)"""
    full = any(k >= 2 for k in kinds)
    per = [f.steer(float(t), full=full) for t in thetas]
    return [[p[k] for p in per] for k in kinds]


def _equal(a, b):
    if torch.is_tensor(a):
        return torch.equal(a, b)
    return np.array_equal(a, b)


def _check(f, thetas, kinds, got):
    want = _per_angle(f, thetas, kinds)
    assert len(got) == len(kinds)
    for k, g, w in zip(kinds, got, want):
        assert len(g) == len(thetas)
        for t in range(len(thetas)):
            # NaN-free inputs: torch.equal is exact
            assert _equal(g[t], w[t]), (k, t, float(thetas[t]))


def _g2(img, opts=None):
    f = cv.SteerableFiltersG2(None)
    for o, v in (opts or {}).items():
        f.set_option(o, v)
    f.setup(img)
    return f


@pytest.mark.parametrize("shape", [(256, 192), (1080, 1920)])
@pytest.mark.parametrize("exact", [False, True])
def test_g2_bank_equals_scalar_calls(shape, exact):
    img = torch.from_numpy(smooth_image(*shape)).to(DEV)
    f = cv.SteerableFiltersG2(None)
    f.set_atan_mode(exact)
    f.setup(img)
    for k in (1, 3, 8):
        th = _thetas(k, seed=k)
        _check(f, th, (0, 1), f.steer_bank(th))
        _check(f, th, (0, 1, 2, 3, 4), f.steer_bank(th, full=True))


def test_g4_bank_equals_scalar_calls():
    img = torch.from_numpy(rand_image(200, 260)).to(DEV)
    f = cv.SteerableFiltersG4(img)
    th = _thetas(8, seed=4)
    _check(f, th, (0, 1), f.steer_bank(th))
    fx = cv.SteerableFiltersG4(img, extensions=True)
    _check(fx, th, (0, 1), fx.steer_bank(th))
    _check(fx, th, (0, 1, 2, 3, 4), fx.steer_bank(th, full=True))
    with pytest.raises(L.CvsError) as e:   # without the extension
        f.steer_bank(th, full=True)
    assert e.value.status == L.E_UNSUPPORTED


@pytest.mark.parametrize("n", [KMAX, KMAX + 1, 100])
def test_chunk_boundaries(n):
    img = torch.from_numpy(rand_image(130, 200, seed=3)).to(DEV)
    f = _g2(img)
    th = np.linspace(-2 * np.pi, 2 * np.pi, n).astype(np.float32)
    th[:5] = np.float32([0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi])
    _check(f, th, (0, 1, 2, 3, 4), f.steer_bank(th, full=True))


def test_kind_subsets():
    img = torch.from_numpy(smooth_image(120, 160)).to(DEV)
    f = _g2(img)
    th = _thetas(5, seed=7)
    for kinds in ((2,), (3, 4), (0,), (1, 3), (4, 2)):
        _check(f, th, kinds, f.steer_bank(th, outputs=kinds))


@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_edge_shapes(shape):
    img = torch.from_numpy(rand_image(*shape, seed=11)).to(DEV)
    f = _g2(img)
    th = _thetas(3, seed=1)
    _check(f, th, (0, 1, 2, 3, 4), f.steer_bank(th, full=True))
    # host (numpy) image: host outputs, the angle-by-angle path
    fh = _g2(rand_image(*shape, seed=11))
    _check(fh, th, (0, 1, 2, 3, 4), fh.steer_bank(th, full=True))


@pytest.mark.parametrize("layout", [0, 1, 2, 3])
def test_state_layouts(layout):
    img = torch.from_numpy(smooth_image(144, 208)).to(DEV)
    f = _g2(img, {L.OPT_STATE_LAYOUT: layout})
    th = _thetas(6, seed=layout)
    _check(f, th, (0, 1, 2, 3, 4), f.steer_bank(th, full=True))
    g4 = cv.SteerableFiltersG4(None, extensions=True)
    g4.set_option(L.OPT_STATE_LAYOUT, layout)
    g4.setup(img)
    _check(g4, th, (0, 1, 2, 3, 4), g4.steer_bank(th, full=True))


def test_frame_of_a_batch():
    frames = torch.stack([torch.from_numpy(rand_image(96, 128, seed=s)) for s in range(3)]).to(DEV)
    f = cv.SteerableFiltersG2(frames[0])
    f.pipeline_batch(frames)
    f.select_frame(2)
    th = _thetas(5, seed=2)
    got = f.steer_bank(th, full=True)
    _check(f, th, (0, 1, 2, 3, 4), got)
    # and it is frame 2's state, not frame 0's
    f.select_frame(0)
    assert not torch.equal(f.steer_bank(th)[0], got[0])


def test_u8_image_and_pipeline_state():
    u8 = torch.from_numpy((rand_image(100, 140, seed=5) * 255).astype(np.uint8)).to(DEV)
    f = _g2(u8)
    th = _thetas(4, seed=9)
    _check(f, th, (0, 1, 2, 3, 4), f.steer_bank(th, full=True))
    img = torch.from_numpy(smooth_image(100, 140)).to(DEV)
    f.pipeline(img)
    _check(f, th, (0, 1, 2, 3, 4), f.steer_bank(th, full=True))


def test_output_placements():
    rows, cols, n = 90, 124, 5
    img = torch.from_numpy(smooth_image(rows, cols)).to(DEV)
    f = _g2(img)
    th = _thetas(n, seed=3)
    # separate allocations (fallback)
    out = [[torch.empty(rows, cols, device=DEV) for _ in range(n)] for _ in range(5)]
    got = f.steer_bank(th, full=True, out=out)
    _check(f, th, (0, 1, 2, 3, 4), got)
    # column ROIs of a wider buffer at irregular offsets (pitch != cols, no constant stride: fallback)
    wide = torch.full((rows, 2 * n * (cols + 7)), float("nan"), device=DEV)
    offs = [k * (cols + 3) + (k * k) % 5 for k in range(n)]
    roi = [[wide[:, o + j * n * (cols + 5): o + j * n * (cols + 5) + cols] for o in offs] for j in range(2)]
    got = f.steer_bank(th, outputs=(3, 4), out=roi)
    _check(f, th, (3, 4), got)
    # host (numpy) outputs
    host = [np.empty((n, rows, cols), np.float32) for _ in range(2)]
    got = f.steer_bank(th, outputs=(0, 1), out=host)
    want = _per_angle(f, th, (0, 1))
    for g, w in zip(got, want):
        for t in range(n):
            assert np.array_equal(g[t], w[t].cpu().numpy())
    # row-interleaved [H][K][W] block: one launch
    blk = [torch.empty(rows, n, cols, device=DEV).permute(1, 0, 2) for _ in range(5)]
    got = f.steer_bank(th, full=True, out=blk)
    _check(f, th, (0, 1, 2, 3, 4), got)


def test_non_default_stream():
    img = torch.from_numpy(smooth_image(160, 256)).to(DEV)
    f = _g2(img)
    th = _thetas(12, seed=12)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = f.steer_bank(th, full=True)
        want = _per_angle(f, th, (0, 1, 2, 3, 4))
    s.synchronize()
    for g, w in zip(got, want):
        for t in range(len(th)):
            assert torch.equal(g[t], w[t])


def test_against_oracle(ora):
    img = rand_image(64, 80, seed=21)
    f = _g2(torch.from_numpy(img).to(DEV))
    b = np.stack([f.basis(p).cpu().numpy() for p in range(7)])
    c = [x.cpu().numpy() for x in f.coefficients()]
    th = np.float32([0.0, 0.4, -2.1, 3.0])
    g, h, e, m, _ = (x.cpu().numpy() for x in f.steer_bank(th, full=True))
    for t, theta in enumerate(th):
        og, oh, oe, om, _ = ora.g2_steer_scalar(b, float(theta), c)
        for got, want in ((g[t], og), (h[t], oh), (e[t], oe), (m[t], om)):
            assert np.abs(got - want).max() <= 1e-5
    f4 = cv.SteerableFiltersG4(torch.from_numpy(img).to(DEV))
    b4 = np.stack([f4.basis(p).cpu().numpy() for p in range(11)])
    g4, h4 = (x.cpu().numpy() for x in f4.steer_bank(th))
    for t, theta in enumerate(th):
        og, oh = ora.g4_steer_scalar(b4, float(theta))
        assert np.abs(g4[t] - og).max() <= 1e-5 and np.abs(h4[t] - oh).max() <= 1e-5


def test_facade_vector_overload(tmp_path):
    exe = os.path.join(str(tmp_path), "test_steer_bank")
    lib = os.path.join(ROOT, "cvsteer_amd")
    if not os.path.exists(os.path.join(lib, "libcvsteer.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cvsteer_amd", "facade"), "-s"])
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-DCVSTEER_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_steer_bank.cpp"), "-L" + lib, "-lcvsteer", "-lcvsteer_hip",
                           "-Wl,-rpath," + lib])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "steer_bank OK" in r.stdout


def _raw(f, thetas, planes):
    th = (C.c_float * max(1, len(thetas)))(*thetas)
    arr = (L.Plane * max(1, len(planes)))(*planes)
    return L.lib().cvs_steer_bank(f._h, th if thetas is not None else None, len(thetas), arr)


def _dev(t):
    return cv.api._plane(t)


def test_errors():
    rows, cols = 64, 96
    img = torch.from_numpy(smooth_image(rows, cols)).to(DEV)
    f = _g2(img)
    a = [torch.empty(rows, cols, device=DEV) for _ in range(10)]
    empty = L.Plane()
    # a kind for some angles only
    assert _raw(f, [0.1, 0.2], [_dev(a[0]), _dev(a[1]), empty, empty, empty, _dev(a[2]), empty, empty, empty, empty]) == L.E_BADARG
    # no kind at all
    assert _raw(f, [0.1], [empty] * 5) == L.E_BADARG
    # two angles sharing one output plane
    assert _raw(f, [0.1, 0.2], [_dev(a[0]), empty, empty, empty, empty, _dev(a[0]), empty, empty, empty, empty]) == L.E_BADARG
    # n = 0, NULL thetas, NULL outs
    assert _raw(f, [], [_dev(a[0])] + [empty] * 4) == L.E_BADARG
    assert L.lib().cvs_steer_bank(f._h, None, 1, (L.Plane * 5)(_dev(a[0]))) == L.E_BADARG
    assert L.lib().cvs_steer_bank(f._h, (C.c_float * 1)(0.5), 1, None) == L.E_BADARG
    # an 8-bit output
    u8 = torch.empty(rows, cols, dtype=torch.uint8, device=DEV)
    p8 = L.Plane(u8.data_ptr(), rows, cols, cols, L.MEM_DEVICE | L.DEPTH_U8)
    assert _raw(f, [0.1], [p8] + [empty] * 4) == L.E_BADARG
    # a plane of another size
    small = torch.empty(rows - 1, cols, device=DEV)
    assert _raw(f, [0.1], [_dev(small)] + [empty] * 4) == L.E_SIZE
    # e after a basis-only setup
    fb = cv.SteerableFiltersG2(None)
    fb.setup(img, flags=cv.SETUP_BASIS)
    assert _raw(fb, [0.1], [empty, empty, _dev(a[0]), empty, empty]) == L.E_STATE
    # no setup
    fn = cv.SteerableFiltersG2(None)
    assert _raw(fn, [0.1], [_dev(a[0])] + [empty] * 4) == L.E_STATE
    # G4 e / magnitude / phase without the extension
    f4 = cv.SteerableFiltersG4(img)
    assert _raw(f4, [0.1], [_dev(a[0]), _dev(a[1]), empty, _dev(a[2]), empty]) == L.E_UNSUPPORTED
    # state dropped by CVS_OPT_PERSIST_STATE = 0
    fp = _g2(img)
    fp.set_persist(False)
    fp.pipeline(img)
    assert _raw(fp, [0.1], [_dev(a[0])] + [empty] * 4) == L.E_STATE
    # Python-side checks: empty or non-1-D thetas never reach the library
    for bad in ([], np.zeros((2, 2), np.float32)):
        with pytest.raises(ValueError):
            f.steer_bank(bad)
    torch.cuda.synchronize()
