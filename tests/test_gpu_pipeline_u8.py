"""GPU tests (-m gpu) of 8-bit pipeline outputs: cvs_pipeline / cvs_pipeline_batch writing byte planes (CVS_DEPTH_U8).

The contract: every byte equals the f32 call followed, per plane, by cvs_normalize_u8 (gain 0) or cvs_convert_u8(plane, gain, 0)
(gain > 0) -- compared with array_equal, no tolerance.  The three-maps launch (edges, dark, bright; no state) quantises in the filter
launch (launch_info u8_out = 1) or reduces min / max there (u8_out = 2); everything else is composed (u8_out = 3)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from cvsteer_amd import _lib as L
from helpers import rand_image, smooth_image

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GAINS = [0.0, 3.0, 1000.0]


@pytest.fixture(scope="module")
def cv():
    import cvsteer_amd
    return cvsteer_amd


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _image(shape, seed, u8=False):
    img = smooth_image(*shape) + 0.05 * rand_image(*shape, seed=seed)
    if u8:
        return (np.clip(img, 0, 1) * 255).astype(np.uint8)
    return img.astype(np.float32)


def _g2(cv, persist=False, gain=0.0):
    f = cv.SteerableFiltersG2(None, 4, 0.67)
    f.set_persist(persist)
    f.set_u8_gain(gain)
    return f


def _expect(f, planes, gain):
    """the composed route on f32 maps: cvs_normalize_u8 / cvs_convert_u8 per plane"""
    return [_np(f.normalize_u8(p) if gain == 0 else f.convert_u8(p, gain)) for p in planes]


def _three_maps(cv, img, gain, persist=False):
    """(bytes of the fused call, bytes of the composed route, u8_out)"""
    import torch
    f = _g2(cv, persist, gain)
    rows, cols = img.shape
    outs = [None] * 5 + [torch.empty((rows, cols), dtype=torch.uint8, device="cuda") for _ in range(3)]
    f.pipeline(img, out=outs)
    u8_out = f.launch_info()["u8_out"]
    ref = f.pipeline(img, out=[None] * 5 + [torch.empty((rows, cols), dtype=torch.float32, device="cuda") for _ in range(3)])
    return [_np(o) for o in outs[5:]], _expect(f, ref[5:], gain), u8_out


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("shape,u8", [((185, 256), True), ((1080, 1920), False), ((1080, 1920), True), ((131, 1021), False),
                                      ((64, 67), True), ((4096, 4096), False)])
def test_three_maps_fused_equal_composed(cv, fish, gain, shape, u8):
    img = fish.astype(np.uint8) if shape == (185, 256) else _image(shape, 7, u8)
    got, want, u8_out = _three_maps(cv, _t(img), gain)
    assert u8_out == (1 if gain > 0 else 2)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


@pytest.mark.parametrize("gain", [0.0, 3.0])
def test_extremes_in_last_column_and_row(cv, gain):
    """an extreme value in the last column and in the last row sets min / max: lanes right of the image and edge rows count right"""
    for where in ("col", "row"):
        img = _image((131, 1021), 3)
        if where == "col":
            img[60, -1] = 500.0
        else:
            img[-1, 400] = -500.0
        got, want, u8_out = _three_maps(cv, _t(img), gain)
        assert u8_out == (1 if gain > 0 else 2)
        for g, w in zip(got, want):
            assert np.array_equal(g, w), where


@pytest.mark.parametrize("gain", GAINS)
def test_constant_and_nonfinite_images(cv, gain):
    got, want, _ = _three_maps(cv, _t(np.full((200, 300), 0.25, np.float32)), gain)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
        if gain == 0:
            assert not g.any()   # max == min: all zeros
    img = _image((200, 300), 5)
    img[10, 10], img[150, 299], img[199, 0] = np.nan, np.inf, -np.inf
    got, want, _ = _three_maps(cv, _t(img), gain)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("n,shape,u8", [(8, (131, 1021), True), (8, (131, 1021), False), (32, (1080, 1920), True), (32, (1080, 1920), False)])
def test_regular_batch(cv, gain, n, shape, u8):
    import torch
    frames = _t(np.stack([_image(shape, 11 + i, u8=u8) for i in range(n)]))
    f = _g2(cv, False, gain)
    got = f.pipeline_batch(frames, outputs=[5, 6, 7], dtype=torch.uint8)
    assert got.dtype == torch.uint8 and f.launch_info()["u8_out"] == (1 if gain > 0 else 2)
    ref = f.pipeline_batch(frames, outputs=[5, 6, 7]).reshape(n * 3, *shape)
    got = _np(got).reshape(n * 3, *shape)
    for i in range(n * 3):
        assert np.array_equal(got[i], _expect(f, [ref[i]], gain)[0]), i


@pytest.mark.parametrize("gain", [0.0, 3.0])
def test_table_batch_and_state_kept_are_composed(cv, gain):
    import torch
    shape = (131, 1021)
    frames = [_t(_image(shape, 20 + i)) for i in range(4)]
    # a list of separate frames (a table batch): composed
    f = _g2(cv, False, gain)
    outs = [torch.empty((3,) + shape, dtype=torch.uint8, device="cuda") for _ in range(4)]
    f.pipeline_batch(frames, out=outs, outputs=[5, 6, 7])
    assert f.launch_info()["u8_out"] == 3
    for i in range(4):
        ref = f.pipeline(frames[i], out=[None] * 5 + [torch.empty(shape, device="cuda") for _ in range(3)])
        for k, w in enumerate(_expect(f, ref[5:], gain)):
            assert np.array_equal(_np(outs[i][k]), w)
    # state kept: composed, and the state equals that of the f32 call
    g = _g2(cv, True, gain)
    got = g.pipeline(frames[0], dtype=torch.uint8)
    assert g.launch_info()["u8_out"] == 3
    st_u8 = [_np(g.basis(p)) for p in range(7)] + [_np(g.getDominantOrientationAngle())]
    ref = g.pipeline(frames[0])
    st_f32 = [_np(g.basis(p)) for p in range(7)] + [_np(g.getDominantOrientationAngle())]
    for a, b in zip(st_u8, st_f32):
        assert np.array_equal(a, b)
    for o, w in zip(got, _expect(g, ref, gain)):
        assert np.array_equal(_np(o), w)


@pytest.mark.parametrize("gain", [0.0, 3.0])
def test_all_outputs_mixed_and_host(cv, gain):
    import torch
    img = _t(_image((185, 256), 4))
    f = _g2(cv, False, gain)
    ref = f.pipeline(img)
    want = _expect(f, ref, gain)
    got = f.pipeline(img, dtype=torch.uint8)                       # all 8 as bytes
    assert f.launch_info()["u8_out"] == 3
    for o, w in zip(got, want):
        assert np.array_equal(_np(o), w)
    mix = [torch.empty((185, 256), dtype=torch.uint8 if k % 2 else torch.float32, device="cuda") for k in range(8)]
    f.pipeline(img, out=mix)                                       # f32 and bytes in one call
    for k in range(8):
        if k % 2:
            assert np.array_equal(_np(mix[k]), want[k])
        else:
            assert np.array_equal(_np(mix[k]), _np(ref[k]))
    host = f.pipeline(_np(img), dtype=np.uint8)                    # host byte planes
    assert all(isinstance(o, np.ndarray) and o.dtype == np.uint8 for o in host)
    for o, w in zip(host, want):
        assert np.array_equal(o, w)


@pytest.mark.parametrize("gain", [0.0, 3.0])
def test_roi_views(cv, gain):
    import torch
    big = _t(_image((300, 1100), 8))
    img = big[20:251, 30:1051]                                     # input step > cols
    f = _g2(cv, False, gain)
    wide = torch.zeros((3, 231, 1100), dtype=torch.uint8, device="cuda")
    outs = [None] * 5 + [wide[k, :, 40:1061] for k in range(3)]   # output step > cols
    f.pipeline(img, out=outs)
    assert f.launch_info()["u8_out"] == (1 if gain > 0 else 2)
    ref = f.pipeline(img, out=[None] * 5 + [torch.empty((231, 1021), device="cuda") for _ in range(3)])
    for o, w in zip(outs[5:], _expect(f, ref[5:], gain)):
        assert np.array_equal(_np(o), w)
    assert not _np(wide[:, :, :40]).any() and not _np(wide[:, :, 1061:]).any()   # nothing written beside the views


@pytest.mark.parametrize("gain", [0.0, 3.0])
def test_orders_and_strip_heights_identical(cv, gain):
    img = _t(_image((1080, 1920), 9))
    results = []
    for order in (0, 1000000, 2000000):
        for strip in (0, 26):
            f = _g2(cv, False, gain)
            f.set_option(L.OPT_AUTOTUNE, 0)
            f.set_option(L.OPT_BLOCK_ORDER, order)
            f.set_strip_rows(strip)
            import torch
            outs = [None] * 5 + [torch.empty((1080, 1920), dtype=torch.uint8, device="cuda") for _ in range(3)]
            f.pipeline(img, out=outs)
            assert f.launch_info()["u8_out"] == (1 if gain > 0 else 2)
            results.append([_np(o) for o in outs[5:]])
    for r in results[1:]:
        for a, b in zip(r, results[0]):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("shape", [(185, 256), (131, 1021), (1080, 1920)])
def test_g4_with_extensions(cv, gain, shape):
    """G4 (extensions on): the per-pixel stage behind the pair launch stores bytes (gain) or reduces min / max (normalise)"""
    import torch
    img = _t(_image(shape, 12))
    f = cv.SteerableFiltersG4(None, 6, 0.5, extensions=True)
    f.set_persist(False)
    f.set_u8_gain(gain)
    got = f.pipeline(img, out=[None] * 5 + [torch.empty(shape, dtype=torch.uint8, device="cuda") for _ in range(3)])
    assert f.launch_info()["u8_out"] == (1 if gain > 0 else 2)
    ref = f.pipeline(img)
    for o, w in zip(got[5:], _expect(f, ref[5:], gain)):
        assert np.array_equal(_np(o), w)
    # a regular batch: one pair launch per frame, ONE per-pixel launch over all frames
    frames = _t(np.stack([_image(shape, 30 + i) for i in range(4)]))
    got = f.pipeline_batch(frames, outputs=[5, 6, 7], dtype=torch.uint8)
    assert f.launch_info()["u8_out"] == (1 if gain > 0 else 2)
    ref = f.pipeline_batch(frames, outputs=[5, 6, 7]).reshape(12, *shape)
    got = _np(got).reshape(12, *shape)
    for i in range(12):
        assert np.array_equal(got[i], _expect(f, [ref[i]], gain)[0]), i
    f.set_persist(True)   # state kept: composed
    got = f.pipeline(img, out=[None] * 5 + [torch.empty(shape, dtype=torch.uint8, device="cuda") for _ in range(3)])
    assert f.launch_info()["u8_out"] == 3
    ref = f.pipeline(img, out=[None] * 5 + [torch.empty(shape, device="cuda") for _ in range(3)])
    for o, w in zip(got[5:], _expect(f, ref[5:], gain)):
        assert np.array_equal(_np(o), w)


@pytest.mark.parametrize("g4", [False, True])
def test_drivers_write_the_composed_files(cv, golden_dir, tmp_path, g4):
    """python -m cvsteer_amd.run and cvsteer-run, with and without --gain, write the bytes of the composed route
    (f32 pipeline, then normalize_u8 / convert_u8 per map)"""
    import torch
    fish = np.load(os.path.join(golden_dir, "fish_u8.npy"))
    rng = np.random.default_rng(9)
    noise = (rng.random((131, 1021)) * 255).astype(np.uint8)
    src = tmp_path / "in"
    src.mkdir()
    np.save(str(src / "fish.npy"), fish)
    np.save(str(src / "noise.npy"), noise)
    lst = tmp_path / "files.txt"
    lst.write_text(str(src / "fish.npy") + "\n" + str(src / "noise.npy") + "\n")
    exe = os.path.join(ROOT, "cvsteer_amd", "cvsteer-run")
    f = cv.SteerableFiltersG4(None, 6, 0.5, extensions=True) if g4 else cv.SteerableFiltersG2(None, 4, 0.67)
    for gain in (0.0, 2.0):
        want = {}
        for base, im in (("fish", fish), ("noise", noise)):
            outs = f.pipeline(torch.from_numpy(im).cuda())
            want[base] = _expect(f, outs[5:], gain)
        extra = (["--g4"] if g4 else []) + (["--gain", "2.0"] if gain else [])
        runs = {"c": [exe, "--input", str(lst), "--ext", ".npy"] + extra,
                "p": [sys.executable, "-m", "cvsteer_amd.run", "--input", str(lst), "--ext", ".npy"] + extra}
        for tag, cmd in runs.items():
            out = tmp_path / ("%s_%g" % (tag, gain))
            out.mkdir()
            r = subprocess.run(cmd + ["--output", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stdout + r.stderr
            for base in want:
                for w, suffix in zip(want[base], ("_edges", "_lines_dark", "_lines_bright")):
                    got = np.load(str(out / (base + suffix + ".npy")))
                    assert got.dtype == np.uint8 and np.array_equal(got, w), (tag, gain, base, suffix)


def _canary(twin):
    path = os.path.join(ROOT, "tools", twin)
    assert os.path.exists(path), "%s missing: run `make -C cvsteer_amd/csrc canary` (or __graft_entry__.build())" % path
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "canary_run.py"), path, "--sections", "u8"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_canary_u8_instances():
    """the hand-counted vmcnt waits of the 8-bit-output instances, checked by the canary twin: 0 stale words, no output row with fewer
    stores than S_ROW, checks that ran in every section; the twin with counts 6 too high is caught on the same sections"""
    r = _canary("libcvsteer_hip_canary.so")
    assert len(r["sections"]) == 12, r
    for name, c in r["sections"].items():
        assert c[2] > 0 and c[3] > 0, (name, c)
        assert c[0] == 0, "stale ring-line words read in %s: %r" % (name, c)
        assert c[1] == 0, "output rows with fewer stores than S_ROW in %s: %r" % (name, c)
    s = _canary("libcvsteer_hip_canary_slack.so")
    assert s["stale"] > 0 and s["short_rows"] == 0, s


def test_errors(cv):
    import torch
    f = _g2(cv)
    for bad in (-1.0, float("nan")):
        with pytest.raises(L.CvsError) as e:
            f.set_u8_gain(bad)
        assert e.value.status == L.E_BADARG
    assert f.u8_gain() == 0.0
    f.set_u8_gain(2.5)
    assert f.u8_gain() == 2.5
    img = _t(_image((64, 80), 1))
    h = L.lib()
    pi = L.Plane(img.data_ptr(), 64, 80, 80 * 4, L.MEM_DEVICE)
    buf = torch.zeros((64, 80), dtype=torch.uint8, device="cuda")
    short = L.Plane(buf.data_ptr(), 64, 80, 79, L.MEM_DEVICE | L.DEPTH_U8)   # step < cols
    arr = (L._PP * 8)(*([None] * 5 + [C_ptr(short)] + [None] * 2))
    assert h.cvs_pipeline(f._h, C_byref(pi), arr) == L.E_SIZE
    over = L.Plane(img.data_ptr(), 64, 80, 80, L.MEM_DEVICE | L.DEPTH_U8)      # bytes on top of the input image
    arr = (L._PP * 8)(*([None] * 5 + [C_ptr(over)] + [None] * 2))
    assert h.cvs_pipeline(f._h, C_byref(pi), arr) == L.E_BADARG
    g4 = cv.SteerableFiltersG4(None, 6, 0.5)
    ok = L.Plane(buf.data_ptr(), 64, 80, 80, L.MEM_DEVICE | L.DEPTH_U8)
    arr = (L._PP * 8)(*([None] * 5 + [C_ptr(ok)] + [None] * 2))
    assert h.cvs_pipeline(g4._h, C_byref(pi), arr) == L.E_UNSUPPORTED


def C_ptr(p):
    import ctypes
    return ctypes.pointer(p)


def C_byref(p):
    import ctypes
    return ctypes.byref(p)
