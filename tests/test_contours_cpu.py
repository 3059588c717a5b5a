"""Contour thinning (cvs_nonmax / cvs_hysteresis) at every layer that exists without a GPU: the public header, the exports of both
libraries, the generated code of the new kernels, and the numpy models the GPU tests hold the kernels against -- including the
direction convention, pinned here on oracle-made maps."""
import os
import re
import subprocess

import numpy as np
import pytest

import contour_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "cvsteer_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def test_header_declares_both():
    text = open(os.path.join(ROOT, "include", "cvsteer_hip.h")).read()
    assert re.search(r"int cvs_nonmax\(cvs_handle h, const cvs_plane\* theta, int n, const cvs_plane\* in, const cvs_plane\* out\);", text)
    assert re.search(r"int cvs_hysteresis\(cvs_handle h, int n, const cvs_plane\* in, float low, float high, const cvs_plane\* out, "
                     r"int\* passes\);", text)
    assert re.search(r"#define CVS_ABI_VERSION 2\b", text)


def test_libraries_export_both():
    import ctypes as C
    from cvsteer_amd import _lib as L
    assert L.SIGNATURES["cvs_nonmax"] == (C.c_int, [C.c_void_p, L._PP, C.c_int, L._PP, L._PP])
    assert L.SIGNATURES["cvs_hysteresis"] == (C.c_int, [C.c_void_p, C.c_int, L._PP, C.c_float, C.c_float, L._PP, L._IP])
    hip = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "cvsteer_amd", "libcvsteer_hip.so")], text=True)
    assert re.search(r" T cvs_nonmax$", hip, re.M) and re.search(r" T cvs_hysteresis$", hip, re.M)
    so = os.path.join(ROOT, "cvsteer_amd", "libcvsteer.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cvsteer_amd", "facade"), "-s"])
    syms = subprocess.check_output(["nm", "-DC", "--defined-only", so], text=True)
    assert "fa::SteerableFiltersG2::nonMaxSuppression(fa::Mat1f const&, fa::Mat1f&)" in syms
    assert "fa::SteerableFiltersG2::hysteresis(fa::Mat1f const&, float, float, fa::Mat1f&)" in syms


def test_null_handle_and_python_surface():
    import cvsteer_amd
    from cvsteer_amd import _lib as L
    planes = (L.Plane * 3)()
    assert L.lib().cvs_nonmax(None, None, 1, planes, planes) == L.E_BADARG
    assert L.lib().cvs_hysteresis(None, 1, planes, 0.0, 1.0, planes, None) == L.E_BADARG
    for name in ("nonmax", "hysteresis", "contours"):
        assert callable(getattr(cvsteer_amd.SteerableFiltersG2, name, None)), name
        assert callable(getattr(cvsteer_amd.SteerableFiltersG4, name, None)), name


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_contour_kernels_use_no_scratch(tmp_path):
    """every instance of the new kernels keeps its values in registers (and LDS): no private segment"""
    path = os.path.join(str(tmp_path), "cvs_kernels_contour.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    "-I" + SRC, "-S", "--cuda-device-only", os.path.join(SRC, "cvs_kernels_contour.hip"), "-o", path], check=True,
                   stderr=subprocess.DEVNULL)
    text = open(path).read()
    scratch = {}
    for blk in text.split("  - .agpr_count:")[1:]:
        nm = re.search(r"\.name:\s+(\S+)", blk)
        ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        if nm and ps:
            scratch[nm.group(1)] = int(ps.group(1))
    nms = {n for n in scratch if "k_nonmax" in n}
    hyst = {n for n in scratch if "k_hyst" in n}
    assert len(nms) == 6 and len(hyst) == 4, sorted(scratch)
    assert all(v == 0 for v in scratch.values()), scratch


# ---- hand-built model cases ----
def _nms(m, theta):
    return M.nonmax([np.float32(m)], np.full(np.shape(m), theta, np.float32))[0]


@pytest.mark.parametrize("theta, ridge", [(0.0, "column"), (np.pi / 2, "row"), (np.pi / 4, "diagonal")])
def test_ridge_5x5(theta, ridge):
    """a one-pixel ridge keeps exactly the ridge: theta = 0 is a vertical contour, pi/2 a horizontal one, +pi/4 runs down-right"""
    r, c = np.mgrid[0:5, 0:5]
    on = {"column": c == 2, "row": r == 2, "diagonal": r == c}[ridge]
    got = _nms(np.where(on, 1.0, 0.0), theta)
    assert np.array_equal(got != 0, on)
    if ridge != "diagonal":   # a graded profile across the ridge too
        dist = np.abs(c - 2) if ridge == "column" else np.abs(r - 2)
        got = _nms(1.0 - 0.2 * dist, theta)
        assert np.array_equal(got != 0, on)
        assert np.array_equal(got[on], np.ones(5, np.float32))


def test_two_pixel_plateau_keeps_one():
    m = np.zeros((3, 6), np.float32)
    m[:, 2:4] = 1.0
    got = _nms(m, 0.0)
    assert np.array_equal(got != 0, np.broadcast_to(np.arange(6) == 2, m.shape))


def test_nan_and_border():
    m = np.float32([[0.5, 1.0, 0.5], [np.nan, 2.0, 0.5], [0.5, 1.0, 0.5]])
    got = _nms(m, 0.0)
    assert got[1, 0] == 0 and got[1, 1] == 0      # NaN in m, and NaN as the backward sample of its neighbour
    assert got[0, 1] == 0                         # 0 * NaN: the diagonal weight is 0, the sample is still NaN
    assert got[2, 1] == 1.0 and got[2, 0] == 0    # outside the image reads as 0.0f
    m[1, 0] = 0.5
    th = np.zeros((3, 3), np.float32)
    assert M.nonmax([m], th)[0][1, 1] == 2.0
    th[1, 1] = np.nan
    assert M.nonmax([m], th)[0][1, 1] == 0


def test_hysteresis_model_chains():
    v = np.zeros((8, 12), np.float32)
    v[2, 1] = 9.0                  # strong seed
    v[2, 2:6] = 5.0                # weak chain attached to it
    v[3, 6] = 5.0                  # ... diagonally (8-connected)
    v[6, 3:9] = 5.0                # a weak chain on its own
    out = M.hysteresis(v, 4.0, 8.0)
    assert out[2, 1] == 255 and (out[2, 2:6] == 255).all() and out[3, 6] == 255
    assert (out[6] == 0).all()
    assert int(np.count_nonzero(out)) == 6
    v[5, 2] = np.nan
    assert M.hysteresis(v, 4.0, 8.0)[5, 2] == 0


# ---- the geometry criteria of the GPU test on the models and the oracle's maps ----
def _oracle_maps(img):
    import oracle
    b = oracle.basis(oracle.KIND_G2, img, 4, 0.67)
    c1, c2, c3, th, _ = oracle.g2_orientation(b)
    _, _, _, mag, ph = oracle.g2_steer_map(b, th, (c1, c2, c3))
    return oracle.find(mag, ph), th


@pytest.mark.parametrize("kind", ["step", "line"])
@pytest.mark.parametrize("polarity", [1, -1])
def test_geometry_on_oracle_maps(kind, polarity):
    for deg in M.ANGLES:
        img, d = M.feature_image(64, deg, kind, polarity)
        maps, th = _oracle_maps(img)
        k = int(np.argmax([np.nanmax(m) for m in maps]))
        thin = M.nonmax([maps[k]], th)[0]
        off, bad, narrow, looked = M.geometry_report(maps[k], thin, d, deg)
        assert looked > 20 and off == 0 and bad == 0 and narrow == 0, (deg, off, bad, narrow, looked)
