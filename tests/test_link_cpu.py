"""The contour chain on the batch axis (cvs_link / cvs_nonmax_batch / cvs_contours_batch) at every layer that exists without a GPU: the
model of cvs_link against the two models it replaces, the public header, the exports and bindings of both libraries, the NULL-handle
calls, the generated code of the link kernels -- no scratch, the border merge touching the parent plane through agent-scope atomics only
-- and the batch driver's --contours argument."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import components_model as CM
import contour_model as HM
import link_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "cvsteer_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
NAMES = ("cvs_link", "cvs_nonmax_batch", "cvs_contours_batch")


def test_model_equals_hysteresis_then_prune():
    cases = M.case_grid()
    assert len(cases) >= 300
    kept_any = 0
    for name, v, low, high, min_area, min_peak in cases:
        got, kept = M.link(v, low, high, min_area, min_peak)
        mask = HM.hysteresis(v, low, high)
        want, wk = CM.prune(mask, min_area, v, min_peak)
        assert kept == wk and np.array_equal(got, want), (name, low, high, min_area, min_peak)
        kept_any += kept > 0
    assert kept_any > 50   # the grid is not a grid of empty answers


def test_model_by_hand():
    v = np.float32([[0.5, 0.9, 0.0, 0.5, 0.5, 0.0, np.nan, 0.9]])
    assert M.link(v, 0.2, 0.7)[0].tolist() == [[255, 255, 0, 0, 0, 0, 0, 255]]
    assert M.link(v, 0.2, 0.7, min_area=2)[1] == 1
    assert M.link(v, 0.2, 0.7, min_area=2)[0].tolist() == [[255, 255, 0, 0, 0, 0, 0, 0]]
    assert M.link(v, 0.2, 0.7, min_peak=1.0)[1] == 0
    assert M.link(v, 0.5, 0.5)[0].tolist() == [[0, 255, 0, 0, 0, 0, 0, 255]]          # low == high: the strong pixels alone
    d = np.float32([[0.9, 0.0], [0.0, 0.3]])
    assert M.link(d, 0.2, 0.7)[0].tolist() == [[255, 0], [0, 255]]                     # diagonals connect


def test_header_declares_the_three():
    text = open(os.path.join(ROOT, "include", "cvsteer_hip.h")).read()
    assert re.search(r"int cvs_link\(cvs_handle h, int n, const cvs_plane\* in, float low, float high, int min_area, float min_peak,\s*"
                     r"const cvs_plane\* out, int32_t\* kept_dev\);", text)
    assert re.search(r"int cvs_nonmax_batch\(cvs_handle h, int frames, int n_maps, const cvs_plane\* theta, const cvs_plane\* in, "
                     r"const cvs_plane\* out\);", text)
    assert re.search(r"int cvs_contours_batch\(cvs_handle h, const cvs_plane\* images, int n, float low, float high, int min_area, "
                     r"float min_peak,\s*const cvs_plane\* outs\);", text)
    assert re.search(r"#define CVS_ABI_VERSION 2\b", text)


def test_libraries_export_and_bind():
    from cvsteer_amd import _lib as L
    assert L.SIGNATURES["cvs_link"] == (C.c_int, [C.c_void_p, C.c_int, L._PP, C.c_float, C.c_float, C.c_int, C.c_float, L._PP, C.c_void_p])
    assert L.SIGNATURES["cvs_nonmax_batch"] == (C.c_int, [C.c_void_p, C.c_int, C.c_int, L._PP, L._PP, L._PP])
    assert L.SIGNATURES["cvs_contours_batch"] == (C.c_int, [C.c_void_p, L._PP, C.c_int, C.c_float, C.c_float, C.c_int, C.c_float, L._PP])
    hip = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "cvsteer_amd", "libcvsteer_hip.so")], text=True)
    for name in NAMES:
        assert re.search(r" T %s$" % name, hip, re.M), name
    so = os.path.join(ROOT, "cvsteer_amd", "libcvsteer.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cvsteer_amd", "facade"), "-s"])
    syms = subprocess.check_output(["nm", "-DC", "--defined-only", so], text=True)
    for cls in ("SteerableFiltersG2", "SteerableFiltersG4"):
        assert "fa::%s::linkContours(fa::Mat1f const&, float, float, int, float, fa::Mat1f&)" % cls in syms
    assert L.lib().cvs_abi_version() == 2


def test_null_handle_and_python_surface():
    import cvsteer_amd
    from cvsteer_amd import _lib as L
    planes = (L.Plane * 3)()
    lib = L.lib()
    assert lib.cvs_link(None, 1, planes, 0.0, 1.0, 0, 0.0, planes, None) == L.E_BADARG
    assert lib.cvs_nonmax_batch(None, 1, 1, None, planes, planes) == L.E_BADARG
    assert lib.cvs_contours_batch(None, planes, 1, 0.0, 1.0, 0, 0.0, planes) == L.E_BADARG
    for name in ("link", "nonmax_batch", "contours_batch", "contours"):
        assert callable(getattr(cvsteer_amd.SteerableFiltersG2, name, None)), name
        assert callable(getattr(cvsteer_amd.SteerableFiltersG4, name, None)), name


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_link_kernels_use_no_scratch_and_the_border_merge_is_atomic(tmp_path):
    path = os.path.join(str(tmp_path), "cvs_kernels_link.s")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                        "-I" + SRC, "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        os.path.join(SRC, "cvs_kernels_link.hip"), "-o", path], check=True, capture_output=True, text=True)
    # what the compiler reports per kernel ...
    names = re.findall(r"remark: Function Name: (\S+)", r.stderr)
    sizes = [int(v) for v in re.findall(r"remark:\s+ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(sizes) and len(names) >= 5, r.stderr[-2000:]
    for stem in ("k_link_table", "k_link_tiles", "k_link_borders", "k_link_stats", "k_link_emit"):
        assert any(stem in n for n in names), (stem, names)
    assert all(v == 0 for v in sizes), dict(zip(names, sizes))
    # ... and what the code object's metadata says
    text = open(path).read()
    scratch = {}
    for blk in text.split("  - .agpr_count:")[1:]:
        nm = re.search(r"\.name:\s+(\S+)", blk)
        ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        if nm and ps:
            scratch[nm.group(1)] = int(ps.group(1))
    assert len(scratch) >= 5 and all(v == 0 for v in scratch.values()), scratch
    # the border merge: every load of it bypasses the CU's L1 (sc1: an agent-scope atomic load), the links are atomic minima, no store
    name = next(n for n in scratch if "k_link_borders" in n)
    body = text[text.index("\n" + name + ":"):]
    body = body[:body.index("s_endpgm")]
    loads = [ln.strip() for ln in body.splitlines() if re.match(r"\s*(global_load|buffer_load|flat_load)", ln)]
    assert len(loads) >= 4, loads
    assert all(re.search(r"\bsc1\b", ln) for ln in loads), [ln for ln in loads if not re.search(r"\bsc1\b", ln)]
    assert re.search(r"_atomic_\w*min", body)
    assert not re.search(r"^\s*(global|buffer|flat)_store", body, re.M)


def test_scratch_bound_is_named():
    text = open(os.path.join(SRC, "cvs_link.h")).read()
    m = re.search(r"constexpr size_t kLinkScratchMax = \(size_t\)1 << (\d+);", text)
    assert m and int(m.group(1)) == 30
    # 32 x 3 planes of 1080p at 12 bytes per pixel cross it, a chain of 4096^2 x 3 does not
    assert 96 * 1080 * 1920 * 12 > 1 << 30 > 3 * 4096 * 4096 * 12


def _run(*args):
    return subprocess.run([sys.executable, "-m", "cvsteer_amd.run", *args], cwd=ROOT, capture_output=True, text=True, timeout=120)


def test_driver_lists_and_validates_contours():
    r = _run("--help")
    assert r.returncode == 0 and "--contours" in r.stdout and "LOW,HIGH[,MIN_AREA[,MIN_PEAK]]" in r.stdout
    for bad in ("5,1", "x", "1", "1,2,3,4,5", "1,2,-3", "1,2,1.5", "nan,2", "1,2,3,nan"):
        r = _run("--input", "nothing.png", "--contours", bad)
        assert r.returncode == 2, (bad, r.returncode, r.stderr)
        assert "--contours" in r.stderr
    from cvsteer_amd import run
    assert run.contours_arg("1,2") == (1.0, 2.0, 0, 0.0)
    assert run.contours_arg("0.5,0.5,7,3.25") == (0.5, 0.5, 7, 3.25)
