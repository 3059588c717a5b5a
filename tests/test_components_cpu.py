"""Contour components (cvs_label / cvs_component_stats / cvs_contour_prune / cvs_contour_points) at every layer that exists without a
GPU: the public header, the exports of both libraries, the Python surface, the generated code of the new kernels -- no scratch, and the
border merge touching the parent plane through agent-scope atomics only -- and the numpy models the GPU tests hold the kernels against."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import components_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "cvsteer_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
NAMES = ("cvs_label", "cvs_component_stats", "cvs_contour_prune", "cvs_contour_points")


def test_header_declares_the_four(tmp_path):
    text = open(os.path.join(ROOT, "include", "cvsteer_hip.h")).read()
    assert re.search(r"int cvs_label\(cvs_handle h, const cvs_plane\* mask, const cvs_plane\* labels, int\* count\);", text)
    assert re.search(r"int cvs_component_stats\(cvs_handle h, const cvs_plane\* labels, int count, const cvs_plane\* weight,\s*"
                     r"cvs_component\* table, int table_mem\);", text)
    assert re.search(r"int cvs_contour_prune\(cvs_handle h, int n, const cvs_plane\* mask, const cvs_plane\* weight, int min_area,\s*"
                     r"float min_peak, const cvs_plane\* out, int\* kept\);", text)
    assert re.search(r"int cvs_contour_points\(cvs_handle h, const cvs_plane\* labels, int32_t\* points, int capacity, int points_mem,\s*"
                     r"int\* n_points\);", text)
    assert re.search(r"enum \{ CVS_DEPTH_S32 = 0x200 \};", text)
    assert re.search(r"#define CVS_ABI_VERSION 2\b", text)
    src = os.path.join(str(tmp_path), "layout.cpp")
    with open(src, "w") as f:
        f.write('#include <stddef.h>\n#include "cvsteer_hip.h"\n'
                'static_assert(sizeof(cvs_component) == 40, "40 bytes");\n'
                'static_assert(offsetof(cvs_component, area) == 0 && offsetof(cvs_component, x0) == 4 && offsetof(cvs_component, y1) == 16, "box");\n'
                'static_assert(offsetof(cvs_component, first_x) == 20 && offsetof(cvs_component, peak_x) == 28 && offsetof(cvs_component, peak) == 36, "rest");\n'
                'static_assert(CVS_DEPTH_S32 == 0x200 && (CVS_DEPTH_S32 & CVS_DEPTH_U8) == 0, "depth flag");\n'
                'int main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), src], check=True)


def test_libraries_export_and_bind():
    from cvsteer_amd import _lib as L
    for name in NAMES:
        assert name in L.SIGNATURES, name
    assert L.SIGNATURES["cvs_label"] == (C.c_int, [C.c_void_p, L._PP, L._PP, L._IP])
    assert L.DEPTH_S32 == 0x200 and C.sizeof(L.Component) == 40
    hip = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "cvsteer_amd", "libcvsteer_hip.so")], text=True)
    for name in NAMES:
        assert re.search(r" T %s$" % name, hip, re.M), name
    so = os.path.join(ROOT, "cvsteer_amd", "libcvsteer.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cvsteer_amd", "facade"), "-s"])
    syms = subprocess.check_output(["nm", "-DC", "--defined-only", so], text=True)
    for cls in ("SteerableFiltersG2", "SteerableFiltersG4"):
        assert "fa::%s::pruneContours(fa::Mat1f const&, fa::Mat1f const&, int, float, fa::Mat1f&)" % cls in syms
        assert "fa::%s::countComponents(fa::Mat1f const&)" % cls in syms


def test_null_handle_and_python_surface():
    import cvsteer_amd
    from cvsteer_amd import _lib as L
    planes = (L.Plane * 3)()
    n = C.c_int(-5)
    lib = L.lib()
    assert lib.cvs_label(None, planes, planes, C.byref(n)) == L.E_BADARG
    assert lib.cvs_component_stats(None, planes, 1, None, None, L.MEM_HOST) == L.E_BADARG
    assert lib.cvs_contour_prune(None, 1, planes, None, 0, 0.0, planes, C.byref(n)) == L.E_BADARG
    assert lib.cvs_contour_points(None, planes, None, 0, L.MEM_HOST, C.byref(n)) == L.E_BADARG
    assert n.value == -5
    for name in ("label", "component_stats", "prune", "contour_points", "contours"):
        assert callable(getattr(cvsteer_amd.SteerableFiltersG2, name, None)), name
        assert callable(getattr(cvsteer_amd.SteerableFiltersG4, name, None)), name
    p = cvsteer_amd.api._plane(np.zeros((5, 12), np.int32)[:, 2:9])
    assert (p.rows, p.cols, p.step, p.mem) == (5, 7, 48, L.MEM_HOST | L.DEPTH_S32)
    assert cvsteer_amd.SteerableFiltersG2.COMPONENT_DTYPE == M.COMPONENT_DTYPE and M.COMPONENT_DTYPE.itemsize == 40


def _isa(tmp_path):
    path = os.path.join(str(tmp_path), "cvs_kernels_components.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    "-I" + SRC, "-S", "--cuda-device-only", os.path.join(SRC, "cvs_kernels_components.hip"), "-o", path], check=True,
                   stderr=subprocess.DEVNULL)
    return open(path).read()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_component_kernels_use_no_scratch_and_the_border_merge_is_atomic(tmp_path):
    text = _isa(tmp_path)
    scratch = {}
    for blk in text.split("  - .agpr_count:")[1:]:
        nm = re.search(r"\.name:\s+(\S+)", blk)
        ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        if nm and ps:
            scratch[nm.group(1)] = int(ps.group(1))
    for stem in ("k_cc_tiles", "k_cc_borders", "k_cc_flatten", "k_cc_relabel", "k_scan_count", "k_scan_partials", "k_scan_apply", "k_stats",
                 "k_prune_stats", "k_prune_emit"):
        assert any(stem in n for n in scratch), (stem, sorted(scratch))
    assert len(scratch) >= 14 and all(v == 0 for v in scratch.values()), scratch
    # the border merge: other workgroups of the same launch change the words it reads, so every load of it must bypass the CU's L1
    # (sc1: what an agent-scope atomic load compiles to), and the links are atomic minima
    name = next(n for n in scratch if "k_cc_borders" in n)
    body = text[text.index("\n" + name + ":"):]
    body = body[:body.index("s_endpgm")]
    loads = [ln.strip() for ln in body.splitlines() if re.match(r"\s*(global_load|buffer_load|flat_load)", ln)]
    assert len(loads) >= 4, loads
    assert all(re.search(r"\bsc1\b", ln) for ln in loads), [ln for ln in loads if not re.search(r"\bsc1\b", ln)]
    assert re.search(r"_atomic_\w*min", body)
    assert not re.search(r"^\s*(global|buffer|flat)_store", body, re.M)   # it writes through the atomics alone


def test_tile_size_is_named_in_the_header():
    text = open(os.path.join(SRC, "cvs_components.h")).read()
    w = re.search(r"constexpr int kCcTileW = (\d+);", text)
    h = re.search(r"constexpr int kCcTileH = (\d+);", text)
    assert w and h and int(w.group(1)) > 0 and int(h.group(1)) > 0


# ---- hand-built model cases ----
def test_two_diagonal_pixels_are_one_component():
    for m in ([[1, 0], [0, 1]], [[0, 1], [1, 0]]):
        lab, n = M.label(np.float32(m))
        assert n == 1 and np.array_equal(lab, np.int32(m))
    lab, n = M.label(np.float32([[1, 0, 1]]))
    assert n == 2 and lab.tolist() == [[1, 0, 2]]


def test_u_shape_and_raster_numbering():
    m = np.float32([[0, 0, 0, 0, 1, 0, 0],
                    [1, 0, 1, 0, 0, 0, 1],
                    [1, 0, 1, 0, 0, 0, 1],
                    [1, 1, 1, 0, 0, 1, 0]])
    lab, n = M.label(m)
    assert n == 3
    assert lab[0, 4] == 1 and lab[1, 0] == 2 and lab[1, 2] == 2 and lab[3, 1] == 2 and lab[1, 6] == 3 and lab[3, 5] == 3
    t = M.stats(lab, n)
    assert t["area"].tolist() == [1, 7, 3]
    assert (t["x0"][1], t["y0"][1], t["x1"][1], t["y1"][1], t["first_x"][1], t["first_y"][1]) == (0, 1, 2, 3, 0, 1)
    assert (t["x0"][2], t["y0"][2], t["x1"][2], t["y1"][2], t["first_x"][2], t["first_y"][2]) == (5, 1, 6, 3, 6, 1)
    assert np.isneginf(t["peak"]).all() and (t["peak_x"] == -1).all()
    pts = M.points(lab)
    assert pts[:3].tolist() == [[4, 0, 1], [0, 1, 2], [2, 1, 2]] and len(pts) == 11


def test_nan_and_negative_pixels_are_background():
    m = np.float32([[np.nan, -1.0, 0.0, -0.0, 1e-30, np.inf]])
    assert M.foreground(m).tolist() == [[False, False, False, False, True, True]]
    assert M.label(m)[1] == 1
    assert M.foreground(np.uint8([[0, 1, 255]])).tolist() == [[False, True, True]]


def test_peak_order_and_ties():
    lab = np.int32([[1, 1, 1, 1, 0, 2, 2, 3]])
    w = np.float32([[-0.0, 0.0, -0.0, 0.0, 9.0, np.nan, -np.inf, np.nan]])
    t = M.stats(lab, 4, w)
    assert t["peak"][0] == 0 and not np.signbit(t["peak"][0]) and (t["peak_x"][0], t["peak_y"][0]) == (1, 0)   # -0.0f < +0.0f, first +0
    assert np.isneginf(t["peak"][1]) and t["peak_x"][1] == 6            # NaN skipped, -inf is a value
    assert np.isneginf(t["peak"][2]) and t["peak_x"][2] == -1           # NaN only: none
    assert t["area"][3] == 0 and t["x0"][3] == -1 and t["first_y"][3] == -1
    w2 = np.float32([[3.0, 7.0, 7.0, 2.0, 0, 0, 0, 0]])
    assert M.stats(lab, 1, w2)["peak_x"][0] == 1                         # the tie goes to the first pixel
    m = np.float32([[1, 1, 1, 1, 0, 1, 1, 0, 1]])
    w3 = np.float32([[-0.0, 0.0, -0.0, 0.0, 9.0, np.nan, -np.inf, 5.0, np.nan]])
    out, kept = M.prune(m, 2)
    assert out.tolist() == [[255, 255, 255, 255, 0, 255, 255, 0, 0]] and kept == 2
    out, kept = M.prune(m, 0, w3, 0.0)
    assert out.tolist() == [[255, 255, 255, 255, 0, 0, 0, 0, 0]] and kept == 1
    out, kept = M.prune(m, 0, w3, -np.inf)
    assert out.tolist() == [[255, 255, 255, 255, 0, 255, 255, 0, 255]] and kept == 3   # "none" is -inf, and -inf >= -inf
