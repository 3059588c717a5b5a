"""GPU tests (-m gpu): every 8-bit output of the library held against the quantisation model of oracle/pyoracle.py.

Each byte plane is compared with np.array_equal against the model (normalize_u8 / convert_u8) applied to the f32 values the library
itself produced -- those are pinned to the oracle elsewhere -- and, every time, against the float64 ideal outside the tie band
(u8_against_ideal).  tests/test_gpu_pipeline_u8.py holds the fused kernels against the composed ones; this file holds both against
the contract, so an edit that changes every copy of the byte arithmetic the same way (rounding, FMA, scale / shift) is seen."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as ora
from cvsteer_amd import _lib as L
from helpers import rand_image, smooth_image
from test_quantize_model_cpu import (distinguishing_inputs, nan_plane, nonfinite_plane, offset_plane, random_plane,
                                     separating_fma_planes, separating_recip_plane, tie_planes)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def cv():
    import cvsteer_amd
    return cvsteer_amd


@pytest.fixture(scope="module")
def eng(cv):
    return cv.SteerableFiltersG2(None)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _model(f32, alpha, beta=0.0):
    """alpha None (or gain 0 in the pipeline's sense, passed as None) = normalise"""
    return ora.normalize_u8(f32) if alpha is None else ora.convert_u8(f32, alpha, beta)


def check_bytes(got, f32, alpha, beta=0.0, what=""):
    """the bytes equal the model on the f32 values, and the float64 ideal outside the tie band (within 1 inside it)"""
    f32 = np.asarray(f32, np.float32)
    got = np.asarray(got)
    assert got.dtype == np.uint8 and got.shape == f32.shape, what
    want = _model(f32, alpha, beta)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError("%s: %d bytes differ from the model; first at %r: got %d, model %d, value %r"
                             % (what, len(bad), i, got[i], want[i], f32[i]))
    off_band, in_band, _ = ora.u8_against_ideal(got, f32, alpha, beta)
    assert off_band == 0 and in_band == 0, (what, off_band, in_band)


def _gain_alpha(gain):
    return None if gain == 0 else gain


# ----------------------------------------------------------------------------- cvs_convert_u8 / cvs_normalize_u8 through ctypes
def _single(h, src, alpha, beta, dst_mem, pad=0, dst_off=0):
    """one cvs_normalize_u8 (alpha None) / cvs_convert_u8 call on the device (or host numpy) plane `src`; dst rows of cols + pad bytes,
    the destination starting dst_off bytes into its buffer; every byte around the plane is a sentinel that must survive"""
    import torch
    rows, cols = src.shape
    step = cols + pad
    if isinstance(src, np.ndarray):
        plane = L.Plane(src.ctypes.data, rows, cols, src.strides[0], L.MEM_HOST)
    else:
        plane = L.Plane(src.data_ptr(), rows, cols, src.stride(0) * 4, L.MEM_DEVICE)
    total = dst_off + rows * step + 8
    if dst_mem == L.MEM_HOST:
        buf = np.full(total, SENTINEL, np.uint8)
        ptr = buf.ctypes.data + dst_off
    else:
        buf = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
        ptr = buf.data_ptr() + dst_off
    lib = L.lib()
    if alpha is None:
        rc = lib.cvs_normalize_u8(h, C.byref(plane), C.c_void_p(ptr), step, dst_mem)
    else:
        rc = lib.cvs_convert_u8(h, C.byref(plane), C.c_float(alpha), C.c_float(beta), C.c_void_p(ptr), step, dst_mem)
    assert rc == 0, lib.cvs_last_error(h)
    assert lib.cvs_sync(h) == 0
    buf = _np(buf)
    body = buf[dst_off:dst_off + rows * step].reshape(rows, step)
    assert (buf[:dst_off] == SENTINEL).all() and (buf[dst_off + rows * step:] == SENTINEL).all()
    assert (body[:, cols:] == SENTINEL).all(), "row padding written"
    return body[:, :cols].copy()


SHAPES = [(1, 1), (1, 7), (7, 1), (3, 5), (33, 65), (1080, 1920)]
PLANES = {"random": random_plane, "offset": offset_plane, "nonfinite": nonfinite_plane, "nan": nan_plane}
MODES = [(None, 0.0), (3.0, 0.0), (0.37, 100.25), (1000.0, -7.5)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", sorted(PLANES))
def test_single_plane_calls_equal_the_model(eng, shape, kind):
    a = PLANES[kind](shape, 5 + shape[0])
    if kind == "offset":
        modes = [(None, 0.0), (85.0, -85000.0)]
    else:
        modes = MODES
    src = _t(a)
    for alpha, beta in modes:
        for mem in (L.MEM_DEVICE, L.MEM_HOST):
            got = _single(eng._h, src, alpha, beta, mem)
            check_bytes(got, a, alpha, beta, (kind, shape, alpha, beta, mem))


def test_tie_and_separating_planes(eng):
    """the exact ties and the inputs that separate mul + add from FMA and 255 / d from 255 * (1 / d) (built as in the CPU tests)"""
    inputs = distinguishing_inputs()
    assert len(inputs) >= 6
    for a, alpha, beta in inputs:
        for mem in (L.MEM_DEVICE, L.MEM_HOST):
            check_bytes(_single(eng._h, _t(a), alpha, beta, mem), a, alpha, beta, (a.shape, alpha, beta, mem))
    # the same planes from the host (uploaded by the call)
    for a, alpha, beta in tie_planes() + separating_fma_planes() + [separating_recip_plane()]:
        check_bytes(_single(eng._h, np.ascontiguousarray(a), alpha, beta, L.MEM_HOST), a, alpha, beta, "host source")


@pytest.mark.parametrize("alpha,beta", [(None, 0.0), (2.5, 0.5)])
def test_roi_sources_and_padded_destinations(eng, alpha, beta):
    """source views with pitch > cols starting at an unaligned column; destinations with dst_step > cols and an unaligned start:
    padding and the bytes around the plane keep their sentinel"""
    big = random_plane((300, 1111), 21)
    big[40, 31] = 900.0                                                # extremes inside the view ...
    big[250, 1059] = -900.0
    big[0, 0], big[299, 1110] = 1e6, -1e6                              # ... and outside it (must not count)
    src_t = _t(big)
    for (r0, r1, c0, c1) in [(20, 251, 31, 1060), (1, 2, 3, 10), (5, 12, 1, 2), (0, 300, 7, 1100)]:
        view = src_t[r0:r1, c0:c1]
        want_src = big[r0:r1, c0:c1]
        for mem in (L.MEM_DEVICE, L.MEM_HOST):
            for pad, off in [(0, 0), (13, 3), (256, 1)]:
                got = _single(eng._h, view, alpha, beta, mem, pad=pad, dst_off=off)
                check_bytes(got, want_src, alpha, beta, (r0, c0, mem, pad, off))


# ----------------------------------------------------------------------------- cvs_normalize_u8_batch / cvs_convert_u8_batch
def _batch_call(h, src_block, alpha, beta, dst_mem, dst_ptrs, dst_step):
    """the planes of a [n, rows, cols] device block view (any row pitch) -> one batch call into dst_ptrs[i]"""
    from cvsteer_amd.api import _PLANE_DTYPE
    n, rows = src_block.shape[0], src_block.shape[1]
    cols = src_block.shape[2]
    planes = np.zeros(n, _PLANE_DTYPE)
    planes["data"] = src_block.data_ptr() + np.arange(n, dtype=np.uint64) * np.uint64(src_block.stride(0) * 4)
    planes["rows"], planes["cols"], planes["step"] = rows, cols, src_block.stride(1) * 4
    planes["mem"] = L.MEM_DEVICE
    dst = np.asarray(dst_ptrs, np.uint64)
    pp = planes.ctypes.data_as(L._PP)
    dp = dst.ctypes.data_as(C.POINTER(C.c_void_p))
    lib = L.lib()
    if alpha is None:
        rc = lib.cvs_normalize_u8_batch(h, pp, n, dp, dst_step, dst_mem)
    else:
        rc = lib.cvs_convert_u8_batch(h, pp, n, C.c_float(alpha), C.c_float(beta), dp, dst_step, dst_mem)
    assert rc == 0, lib.cvs_last_error(h)
    assert lib.cvs_sync(h) == 0


def _ranged_block(n, rows, cols, seed):
    """n planes, each with its own range (a wrong min / max slot shows), a NaN in some; offsets stay small against the spans, so a
    plane's min maps to 0 and its max to 255 exactly"""
    rng = np.random.default_rng(seed)
    i = np.arange(n).reshape(n, 1, 1)
    a = (rng.random((n, rows, cols)) * (1.0 + i % 13) - 0.5 * (7 * i % 101)).astype(np.float32)
    a[::5, 0, 0] = np.nan
    return a


def _check_block(got, block, alpha, beta, what):
    if alpha is None:
        for i in range(block.shape[0]):
            check_bytes(got[i], block[i], None, 0.0, (what, i))
    else:
        check_bytes(got, block, alpha, beta, what)


@pytest.mark.parametrize("n", [3, 8, 19])
@pytest.mark.parametrize("layout", ["vec", "cols%4=1", "cols%4=2", "cols%4=3", "dst_off", "odd_pitch"])
def test_batch_calls_equal_the_model(eng, n, layout):
    """k_minmax_n / k_to_u8_n: the four-pixel instances (cols % 4 == 0, aligned) and the one-pixel ones (cols % 4 in {1, 2, 3}, a
    destination 1..3 bytes off alignment, an odd source pitch); n < 8 and n >= 8 (the gy clamp); host and device destinations"""
    import torch
    rows, cols = 37, {"vec": 132, "cols%4=1": 129, "cols%4=2": 130, "cols%4=3": 131, "dst_off": 132, "odd_pitch": 132}[layout]
    pitch = 133 if layout == "odd_pitch" else cols
    block = _ranged_block(n, rows, pitch, 30 + n)
    dev = _t(block)[:, :, :cols]
    want_src = block[:, :, :cols]
    off = 2 if layout == "dst_off" else 0
    for alpha, beta in [(None, 0.0), (1.7, 0.0), (0.6, 127.5)]:
        # device destinations at a constant stride: the one-launch path straight into them
        buf = torch.full((off + n * rows * cols + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
        ptrs = [buf.data_ptr() + off + i * rows * cols for i in range(n)]
        _batch_call(eng._h, dev, alpha, beta, L.MEM_DEVICE, ptrs, cols)
        b = _np(buf)
        assert (b[:off] == SENTINEL).all() and (b[off + n * rows * cols:] == SENTINEL).all()
        _check_block(b[off:off + n * rows * cols].reshape(n, rows, cols), want_src, alpha, beta, (layout, n, alpha, "device"))
        # host destinations with padded rows (staged, copied row by row)
        host = np.full((n, rows, cols + 3), SENTINEL, np.uint8)
        _batch_call(eng._h, dev, alpha, beta, L.MEM_HOST, [host[i].ctypes.data for i in range(n)], cols + 3)
        assert (host[:, :, cols:] == SENTINEL).all()
        _check_block(host[:, :, :cols], want_src, alpha, beta, (layout, n, alpha, "host"))


@pytest.mark.parametrize("cols", [4, 3])
def test_batch_of_65537_planes_crosses_the_grid_z_chunks(eng, cols):
    """65537 equal 2 x cols planes in ONE device allocation at a constant stride: to_u8_batch takes its one-launch path (regular device
    planes), and launch_to_u8_n splits the planes at 65535 -- the second chunk's min / max slots (mm + 2 z0) and destinations
    (dst + z0 stride) are exercised.  Host destinations lie back to back (the packed staging, one copy); device destinations lie at a
    constant stride (straight into them).  cols 4 takes the four-pixel instances, cols 3 the one-pixel ones."""
    import torch
    n, rows = 65537, 2
    block = _ranged_block(n, rows, cols, 7)
    dev = _t(block)
    for alpha, beta in [(None, 0.0), (3.0, 1.5)]:
        host = np.full((n, rows, cols), SENTINEL, np.uint8)
        _batch_call(eng._h, dev, alpha, beta, L.MEM_HOST, host.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(rows * cols),
                    cols)
        ddst = torch.full((n, rows, cols), SENTINEL, dtype=torch.uint8, device="cuda")
        _batch_call(eng._h, dev, alpha, beta, L.MEM_DEVICE, ddst.data_ptr() + np.arange(n, dtype=np.uint64) * np.uint64(rows * cols),
                    cols)
        got_d = _np(ddst)
        assert np.array_equal(host, got_d)
        if alpha is None:
            # every plane's own range: its min maps to 0 and its max to 255 (a plane that read another's slot would not)
            fin = np.where(np.isnan(block), np.inf, block).reshape(n, -1)
            assert (host.reshape(n, -1)[np.arange(n), fin.argmin(1)] == 0).all()
            fin = np.where(np.isnan(block), -np.inf, block).reshape(n, -1)
            assert (host.reshape(n, -1)[np.arange(n), fin.argmax(1)] == 255).all()
            want = np.stack([ora.normalize_u8(block[i]) for i in range(n)])
            assert np.array_equal(host, want)
            for i in (0, 1, 65534, 65535, 65536):
                check_bytes(host[i], block[i], None, 0.0, i)
        else:
            check_bytes(host, block, alpha, beta, "convert")


# ----------------------------------------------------------------------------- the three-maps pipeline (u8_out 1 and 2)
def _image(shape, seed, u8=False):
    img = smooth_image(*shape) + 0.05 * rand_image(*shape, seed=seed)
    if u8:
        return (np.clip(img, 0, 1) * 255).astype(np.uint8)
    return img.astype(np.float32)


def _fused_expected(shape):
    return shape[0] >= 13 and shape[1] >= 5          # fast geometry of the default width: else composed


def _handle(cv, gain, width=None, spacing=None):
    f = cv.SteerableFiltersG2(None, width, spacing)
    f.set_persist(False)
    f.set_u8_gain(gain)
    return f


def _three_maps_vs_model(f, img, gain, fused):
    import torch
    rows, cols = img.shape
    outs = [None] * 5 + [torch.empty((rows, cols), dtype=torch.uint8, device="cuda") for _ in range(3)]
    f.pipeline(img, out=outs)
    assert f.launch_info()["u8_out"] == ((1 if gain > 0 else 2) if fused else 3)
    ref = f.pipeline(img, out=[None] * 5 + [torch.empty((rows, cols), dtype=torch.float32, device="cuda") for _ in range(3)])
    for k in range(3):
        check_bytes(_np(outs[5 + k]), _np(ref[5 + k]), _gain_alpha(gain), 0.0, (img.shape, gain, k))


GAINS = [0.0, 0.5, 3.0, 1000.0]


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("shape,u8", [((1, 1), False), ((7, 1), False), ((17, 31), False), ((17, 31), True), ((131, 1021), False),
                                      ((185, 256), True), ((1080, 1920), False), ((1080, 1920), True), ((4096, 4096), False)])
def test_three_maps_single_image(cv, fish, gain, shape, u8):
    img = fish.astype(np.uint8) if shape == (185, 256) else _image(shape, 7, u8)
    f = _handle(cv, gain)
    _three_maps_vs_model(f, _t(img), gain, _fused_expected(shape))
    if _fused_expected(shape):
        assert f.launch_info()["literal_taps"] == 1


@pytest.mark.parametrize("gain", [0.0, 3.0])
def test_three_maps_argument_taps_and_other_widths(cv, gain):
    """spacing 0.5 at the default width: the argument-tap instance, still fused; width 6: composed"""
    img = _t(_image((131, 1021), 4))
    f = _handle(cv, gain, 4, 0.5)
    _three_maps_vs_model(f, img, gain, True)
    assert f.launch_info()["literal_taps"] == 0
    lit = _handle(cv, gain)
    _three_maps_vs_model(lit, img, gain, True)
    assert lit.launch_info()["literal_taps"] == 1
    _three_maps_vs_model(_handle(cv, gain, 6, 0.5), img, gain, False)


@pytest.mark.parametrize("n,shape,u8,gain,spacing", [(8, (131, 1021), u8, g, None) for u8 in (False, True) for g in GAINS] +
                         [(8, (131, 1021), False, g, 0.5) for g in (0.0, 3.0)] +
                         [(32, (1080, 1920), u8, g, None) for u8 in (False, True) for g in (0.0, 3.0)])
def test_three_maps_batch(cv, n, shape, u8, gain, spacing):
    """a regular frame batch (literal taps, or argument taps at spacing 0.5); the last frame carries extremes in its last row and
    its last column (its own min / max)"""
    import torch
    frames = np.stack([_image(shape, 11 + i, u8=u8) for i in range(n)])
    frames[-1, -1, shape[1] // 2] = 0 if u8 else -40.0
    frames[-1, shape[0] // 2, -1] = 255 if u8 else 60.0
    frames = _t(frames)
    f = _handle(cv, gain, 4 if spacing else None, spacing)
    got = f.pipeline_batch(frames, outputs=[5, 6, 7], dtype=torch.uint8)
    assert f.launch_info()["u8_out"] == (1 if gain > 0 else 2)
    assert f.launch_info()["literal_taps"] == (0 if spacing else 1)
    got = _np(got).reshape(n * 3, *shape)
    ref = _np(f.pipeline_batch(frames, outputs=[5, 6, 7])).reshape(n * 3, *shape)
    for i in range(n * 3):
        check_bytes(got[i], ref[i], _gain_alpha(gain), 0.0, (n, shape, gain, spacing, i))


@pytest.mark.parametrize("gain", [0.0, 0.5, 1000.0])
def test_three_maps_extremes_in_last_row_and_column(cv, gain):
    for where in ("col", "row", "corner"):
        img = _image((131, 1021), 3)
        if where in ("col", "corner"):
            img[60 if where == "col" else -1, -1] = 500.0
        if where in ("row", "corner"):
            img[-1, 400] = -500.0
        _three_maps_vs_model(_handle(cv, gain), _t(img), gain, True)


# ----------------------------------------------------------------------------- G4 with extensions (k_g4_pipeline U8 1 / 2)
@pytest.mark.parametrize("gain", [0.0, 0.5, 3.0])
@pytest.mark.parametrize("shape", [(70, 110), (1080, 1920)])
def test_g4_pipeline_u8(cv, gain, shape):
    """(70, 110): cols % 4 != 0, the dword instance; (1080, 1920): the float4 instance; then a batch of frames"""
    import torch
    img = _image(shape, 12)
    img[-1, -1] = 9.0
    f = cv.SteerableFiltersG4(None, 6, 0.5, extensions=True)
    f.set_persist(False)
    f.set_u8_gain(gain)
    got = f.pipeline(_t(img), out=[None] * 5 + [torch.empty(shape, dtype=torch.uint8, device="cuda") for _ in range(3)])
    assert f.launch_info()["u8_out"] == (1 if gain > 0 else 2)
    ref = f.pipeline(_t(img))
    for k in range(5, 8):
        check_bytes(_np(got[k]), _np(ref[k]), _gain_alpha(gain), 0.0, (shape, gain, k))
    n = 4
    frames = np.stack([_image(shape, 30 + i) for i in range(n)])
    frames[-1, -1, 3] = -9.0
    frames = _t(frames)
    got = _np(f.pipeline_batch(frames, outputs=[5, 6, 7], dtype=torch.uint8)).reshape(n * 3, *shape)
    assert f.launch_info()["u8_out"] == (1 if gain > 0 else 2)
    ref = _np(f.pipeline_batch(frames, outputs=[5, 6, 7])).reshape(n * 3, *shape)
    for i in range(n * 3):
        check_bytes(got[i], ref[i], _gain_alpha(gain), 0.0, (shape, gain, "batch", i))


# ----------------------------------------------------------------------------- the composed route (u8_out 3)
@pytest.mark.parametrize("gain", [0.0, 3.0])
def test_composed_route(cv, gain):
    """state kept (device planes) and host planes: composed, against the model"""
    import torch
    img = _image((185, 256), 4)
    f = cv.SteerableFiltersG2(None)
    f.set_u8_gain(gain)
    got = f.pipeline(_t(img), dtype=torch.uint8)                   # state kept (the default)
    assert f.launch_info()["u8_out"] == 3
    ref = f.pipeline(_t(img))
    for k in range(8):
        check_bytes(_np(got[k]), _np(ref[k]), _gain_alpha(gain), 0.0, ("state", k))
    host = f.pipeline(img, dtype=np.uint8)                           # host planes
    assert f.launch_info()["u8_out"] == 3
    assert all(isinstance(o, np.ndarray) for o in host)
    for k in range(8):
        check_bytes(host[k], _np(ref[k]), _gain_alpha(gain), 0.0, ("host", k))


# ----------------------------------------------------------------------------- drivers and the batch layer
@pytest.mark.parametrize("g4", [False, True])
def test_drivers_write_the_model_bytes(cv, golden_dir, tmp_path, g4):
    """cvsteer-run and python -m cvsteer_amd.run (with and without --g4, with and without --gain): the written maps equal the
    model on the f32 pipeline outputs"""
    import torch
    fish = np.load(os.path.join(golden_dir, "fish_u8.npy"))
    noise = (np.random.default_rng(9).random((131, 1021)) * 255).astype(np.uint8)
    src = tmp_path / "in"
    src.mkdir()
    np.save(str(src / "fish.npy"), fish)
    np.save(str(src / "noise.npy"), noise)
    lst = tmp_path / "files.txt"
    lst.write_text(str(src / "fish.npy") + "\n" + str(src / "noise.npy") + "\n")
    exe = os.path.join(ROOT, "cvsteer_amd", "cvsteer-run")
    f = cv.SteerableFiltersG4(None, 6, 0.5, extensions=True) if g4 else cv.SteerableFiltersG2(None, 4, 0.67)
    maps = {base: [_np(o) for o in f.pipeline(torch.from_numpy(im).cuda())[5:]] for base, im in (("fish", fish), ("noise", noise))}
    for gain in (0.0, 2.0):
        extra = (["--g4"] if g4 else []) + (["--gain", "2.0"] if gain else [])
        runs = {"c": [exe, "--input", str(lst), "--ext", ".npy"] + extra,
                "p": [sys.executable, "-m", "cvsteer_amd.run", "--input", str(lst), "--ext", ".npy"] + extra}
        for tag, cmd in runs.items():
            out = tmp_path / ("%s_%g" % (tag, gain))
            out.mkdir()
            r = subprocess.run(cmd + ["--output", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stdout + r.stderr
            for base, planes in maps.items():
                for plane, suffix in zip(planes, ("_edges", "_lines_dark", "_lines_bright")):
                    got = np.load(str(out / (base + suffix + ".npy")))
                    check_bytes(got, plane, _gain_alpha(gain), 0.0, (tag, gain, base, suffix))


@pytest.mark.parametrize("world", [1, 3])
def test_batch_run_bytes_equal_the_model(cv, world):
    """cvs_batch_run with 8-bit host output planes (NativeBatch.run_to_u8, the one-card rehearsal for world 3) and the two-step
    flow: every byte is the model on the single-engine f32 maps"""
    import torch
    from cvsteer_amd import batch
    n, rows, cols = 7, 75, 210
    u8 = np.random.default_rng(11).integers(0, 256, (n, rows, cols), dtype=np.uint8)
    u8[-1, -1, -1] = 255
    ref = _np(cv.SteerableFiltersG2(None).pipeline_batch(torch.from_numpy(u8.astype(np.float32)).cuda(), outputs=(5, 6, 7)))
    nb = batch.NativeBatch.local((0,) * world)
    for persist in (False, True):
        nb.set_persist(persist)
        for gain in (0.0, 3.0):
            for run in (nb.run_to_u8, nb.run_to_u8_two_step):
                q, _ = run(u8, gain=gain)
                assert q.shape == (n, 3, rows, cols)
                for i in range(n):
                    for k in range(3):
                        check_bytes(q[i, k], ref[i, k], _gain_alpha(gain), 0.0, (world, persist, gain, run.__name__, i, k))
    nb.close()
