"""GPU tests (-m gpu) of the G4 caller pipeline (CVS_OPT_G4_EXTENSIONS = 1): cvs_pipeline / cvs_pipeline_batch /
cvs_batch_run and the batch drivers' --g4 on the G4/H4 bank.

The contract: every output and every state plane equals, bit for bit, what the same handle gives from
setup(FULL) -> steer(None, full=True) -> find(magnitude | e, phase); against the CPU oracle the tolerances of
test_gpu_parity.py::test_g4_extension_orientation_and_full_steer hold."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cvsteer_amd import _lib as L
from helpers import angle_diff, rand_image, smooth_image

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5


@pytest.fixture(scope="module")
def cv():
    import cvsteer_amd
    return cvsteer_amd


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _g4(cv, find_on=0, atan=0):
    f = cv.SteerableFiltersG4(None, 6, 0.5, extensions=True)
    f.set_option(L.OPT_FIND_ON, find_on)
    f.set_option(L.OPT_ATAN_MODE, atan)
    return f


def _state(f):
    """the 11 basis planes, then C1, C2, C3, theta, strength"""
    return [_np(f.basis(p)) for p in range(11)] + [_np(c) for c in f.coefficients()] + \
           [_np(f.getDominantOrientationAngle()), _np(f.getDominantOrientationStrength())]


def _composed(cv, f, img):
    """the four-call composition the pipeline must reproduce -> (8 outputs, 16 state planes)"""
    f.setup(img, cv.SETUP_FULL)
    g, h, e, m, p = f.steer(None, full=True)
    ed, dk, br = f.find(e if f.get_option(L.OPT_FIND_ON) else m, p)
    return [_np(o) for o in (g, h, e, m, p, ed, dk, br)], _state(f)


def _image(shape, seed, device):
    img = (smooth_image(*shape) + 0.05 * rand_image(*shape, seed=seed)).astype(np.float32)
    if device:
        import torch
        return torch.from_numpy(img).cuda()
    return img


def _assert_equal(got, want, what):
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and np.array_equal(a, b), (what, k, float(np.abs(a - b).max()))


# ----------------------------------------------------------------------------- 1. composition identity
@pytest.mark.parametrize("shape,device,find_on,atan", [
    ((70, 110), True, 0, 0), ((70, 110), True, 1, 0), ((70, 110), True, 0, 1), ((70, 110), True, 1, 1),
    ((33, 65), True, 0, 0), ((33, 65), True, 1, 1),            # ragged: the dword path
    ((1080, 1920), True, 0, 0), ((1080, 1920), True, 1, 1),
    ((2048, 2048), False, 0, 0),                               # host numpy image and host outputs
])
def test_pipeline_equals_composition(cv, shape, device, find_on, atan):
    img = _image(shape, 31 + shape[0], device)
    f = _g4(cv, find_on, atan)
    want, want_state = _composed(cv, f, img)
    outs = f.pipeline(img)
    _assert_equal([_np(o) for o in outs], want, "outputs")
    _assert_equal(_state(f), want_state, "state")


def test_pipeline_fish_fixture(cv, fish):
    import torch
    for img in (fish, torch.from_numpy(fish).cuda(), torch.from_numpy(fish.astype(np.uint8)).cuda()):
        f = _g4(cv)
        want, want_state = _composed(cv, f, img)
        outs = f.pipeline(img)
        _assert_equal([_np(o) for o in outs], want, "outputs")
        _assert_equal(_state(f), want_state, "state")


# ----------------------------------------------------------------------------- 2. oracle parity
@pytest.mark.parametrize("atan", [0, 1])
def test_pipeline_matches_oracle(cv, ora, atan):
    img = _image((70, 110), 77, False)
    f = _g4(cv, 0, atan)
    g, h, e, m, p, ed, dk, br = [_np(o) for o in f.pipeline(img)]
    st = _state(f)
    b = np.stack(st[:11])
    assert np.abs(b - ora.basis(4, img, 6, 0.5, f64=True)).max() <= TOL
    assert np.abs(b - ora.basis(4, img, 6, 0.5)).max() <= TOL
    o1, o2, o3, oth, ost = ora.g4_orientation(b, atan)
    scale = max(1.0, float(np.abs(o1).max()))
    for got, want in zip(st[11:14] + [st[15]], (o1, o2, o3, ost)):
        assert np.abs(got - want).max() <= 1e-6 * scale
    ok = ost > 1e-3 * scale
    assert angle_diff(st[14], oth, np.pi)[ok].max() <= TOL
    og, oh = ora.g4_steer_map(b, st[14])                        # steered at the GPU's theta
    assert np.abs(g - og).max() <= TOL and np.abs(h - oh).max() <= TOL
    th2 = 2.0 * st[14].astype(np.float64)
    want_e = st[11] + st[12] * np.cos(th2) + st[13] * np.sin(th2)
    assert np.abs(e - want_e).max() <= TOL * scale
    om, op = ora.mag_phase(og, oh, atan)
    assert np.abs(m - om).max() <= TOL
    assert angle_diff(p, op, 2 * np.pi)[om > 1e-3].max() <= 2e-5
    for got, want in zip((ed, dk, br), ora.find(m, p)):         # fed the same magnitude / phase
        assert np.abs(got - want).max() <= TOL * max(1.0, float(np.abs(want).max()))


# ----------------------------------------------------------------------------- 3. optional outputs
@pytest.mark.parametrize("sel", [(5, 6, 7), (0, 1), (2,), (3, 4, 7), (0, 2, 5), (4,)])
def test_optional_outputs(cv, sel):
    import torch
    img = _image((70, 110), 5, True)
    f = _g4(cv)
    want, _ = _composed(cv, f, img)
    blk = torch.full((8, 70, 110), -1234.5, dtype=torch.float32, device="cuda")
    outs = f.pipeline(img, out=[blk[k] if k in sel else None for k in range(8)])
    for k in range(8):
        if k in sel:
            assert np.array_equal(_np(outs[k]), want[k]), k
        else:
            assert outs[k] is None and bool((blk[k] == -1234.5).all()), k


# ----------------------------------------------------------------------------- 4. no-state mode
def test_no_state_mode(cv):
    img = _image((70, 110), 9, True)
    f = _g4(cv)
    want, _ = _composed(cv, f, img)
    f.set_persist(False)
    _assert_equal([_np(o) for o in f.pipeline(img)], want, "outputs")
    for read in (lambda: f.basis(0), f.getDominantOrientationAngle, f.coefficients):
        with pytest.raises(cv.CvsError) as ex:
            read()
        assert ex.value.status == L.E_STATE
    f.set_persist(True)
    f.pipeline(img)
    assert f.basis(0) is not None


# ----------------------------------------------------------------------------- 5. frame batches
def _singles(cv, frames):
    outs, states = [], []
    for fr in frames:
        f = _g4(cv)
        outs.append([_np(o) for o in f.pipeline(fr)])
        states.append(_state(f))
    return outs, states


def _check_batch(f, out, outs, states):
    for i in range(len(outs)):
        _assert_equal([_np(out[i][k]) for k in range(8)], outs[i], ("frame", i))
        f.select_frame(i)
        _assert_equal(_state(f), states[i], ("state", i))


def test_batch_regular_block(cv):
    import torch
    n = 5
    frames = torch.stack([_image((70, 112), 50 + i, True) for i in range(n)])
    outs, states = _singles(cv, list(frames))
    f = _g4(cv)
    out = f.pipeline_batch(frames)
    assert tuple(out.shape) == (n, 8, 70, 112)
    _check_batch(f, out, outs, states)
    # three maps only, no state
    g = _g4(cv)
    g.set_persist(False)
    three = g.pipeline_batch(frames, outputs=(5, 6, 7))
    for i in range(n):
        for j, k in enumerate((5, 6, 7)):
            assert np.array_equal(_np(three[i, j]), outs[i][k]), (i, k)
    with pytest.raises(cv.CvsError):
        g.basis(0)


def test_batch_table_u8_and_host(cv):
    import torch
    n = 4
    planes = [_image((45, 67), 60 + i, True) for i in range(n)]     # unrelated allocations
    outs, states = _singles(cv, planes)
    f = _g4(cv)
    out = [[torch.empty((45, 67), dtype=torch.float32, device="cuda") for _ in range(8)] for _ in range(n)]
    f.pipeline_batch(planes, out=out)
    _check_batch(f, out, outs, states)
    # host numpy frames
    host = np.stack([_np(p) for p in planes])
    f = _g4(cv)
    out = f.pipeline_batch(host)
    assert isinstance(out, np.ndarray)
    _check_batch(f, out, outs, states)
    # 8-bit device frames, one block
    u8 = torch.stack([(p * 40).clamp(0, 255).to(torch.uint8) for p in planes])
    outs8, states8 = _singles(cv, list(u8))
    f = _g4(cv)
    out = f.pipeline_batch(u8)
    _check_batch(f, out, outs8, states8)


# ----------------------------------------------------------------------------- 6. multi-GPU batch, rehearsed on one card
def test_native_batch_g4(cv):
    import torch
    from cvsteer_amd.batch import NativeBatch
    n = 6
    frames = torch.stack([_image((64, 96), 80 + i, True) for i in range(n)]).contiguous()
    outs, _ = _singles(cv, list(frames))
    nb = NativeBatch.local((0, 0), kind=cv.KIND_G4, width=6, spacing=0.5)
    with pytest.raises(cv.CvsError) as ex:      # extensions off
        nb.run(frames, n, (64, 96))
    assert ex.value.status == L.E_UNSUPPORTED
    nb.set_g4_extensions(True)
    got, _ = nb.run(frames, n, (64, 96), outputs=tuple(range(8)))
    for i in range(n):
        _assert_equal([_np(got[i, k]) for k in range(8)], outs[i], ("frame", i))
    host = _np(frames)
    u8, _ = nb.run_to_u8(host)
    f = _g4(cv)
    for i in range(n):
        for j, k in enumerate((5, 6, 7)):
            assert np.array_equal(u8[i, j], _np(f.normalize_u8(torch.from_numpy(outs[i][k]).cuda()))), (i, k)
    nb.close()


# ----------------------------------------------------------------------------- 7. batch drivers
def test_batch_drivers_g4(cv, tmp_path, golden_dir):
    import torch
    fish = np.load(os.path.join(golden_dir, "fish_u8.npy"))
    src = tmp_path / "fish.npy"
    np.save(str(src), fish)
    f = _g4(cv)
    outs = f.pipeline(torch.from_numpy(fish).cuda())
    want = [_np(f.normalize_u8(outs[k])) for k in (5, 6, 7)]
    exe = os.path.join(ROOT, "cvsteer_amd", "cvsteer-run")
    runs = {"c": [exe, "--g4", "--input", str(src), "--output", str(tmp_path / "c"), "--ext", ".npy"],
            "p": [sys.executable, "-m", "cvsteer_amd.run", "--g4", "--input", str(src), "--output", str(tmp_path / "p"), "--ext", ".npy"]}
    for tag, cmd in runs.items():
        (tmp_path / tag).mkdir()
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        for w, suffix in zip(want, ("_edges", "_lines_dark", "_lines_bright")):
            got = np.load(str(tmp_path / tag / ("fish" + suffix + ".npy")))
            assert got.dtype == np.uint8 and np.array_equal(got, w), (tag, suffix)


# ----------------------------------------------------------------------------- 8. extensions off: unchanged
def test_extensions_off_unsupported(cv):
    import torch
    img = _image((40, 60), 3, True)
    f = cv.SteerableFiltersG4(None, 6, 0.5)
    calls = [lambda: f.pipeline(img), lambda: f.pipeline_batch(torch.stack([img, img])),
             lambda: f.find(img, img), lambda: f.normalize_u8(img), lambda: f.set_persist(False), lambda: f.select_frame(0)]
    for call in calls:
        with pytest.raises(cv.CvsError) as ex:
            call()
        assert ex.value.status == L.E_UNSUPPORTED
