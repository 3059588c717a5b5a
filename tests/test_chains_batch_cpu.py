"""Contour chains and sub-pixel chain points on the batch axis (cvs_contour_chains_batch, cvs_chain_refine_batch) at every layer that exists
without a GPU: the public header, the exports of the library and the unit lists every twin of it is built from, the Python surface, the
NULL-handle calls, the generated code of the new kernels (no scratch), and the model the GPU tests hold the kernels against -- the per-plane
model concatenated, cross-checked against one run of the single-image model on the stacked planes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import chains_batch_model as M
import chains_model as CM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "cvsteer_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
NAMES = ("cvs_contour_chains_batch", "cvs_chain_refine_batch")


def test_header_declares_both_calls(tmp_path):
    text = open(os.path.join(ROOT, "include", "cvsteer_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int cvs_contour_chains_batch\(cvs_handle h, int n, const cvs_plane\* masks,\s*int32_t\* points, int point_capacity,\s*"
                     r"cvs_chain\* chains, int chain_capacity,\s*int32_t\* ranges,\s*int mem,\s*int\* n_points, int\* n_chains\);", plain)
    assert re.search(r"int cvs_chain_refine_batch\(cvs_handle h, int frames, int n_maps,\s*const cvs_plane\* maps,\s*const cvs_plane\* theta,\s*"
                     r"const int32_t\* points, int n_points,\s*const int32_t\* ranges,\s*float\* xy, float\* strength, int mem\);", plain)
    assert re.search(r"#define CVS_ABI_VERSION 2\b", text)
    assert "2.0 GB" in text and "2^28" in text                                # the header says what the stacked block costs and where it ends
    src = os.path.join(str(tmp_path), "use.cpp")
    with open(src, "w") as f:
        f.write('#include "cvsteer_hip.h"\n'
                'int (*chains)(cvs_handle, int, const cvs_plane*, int32_t*, int, cvs_chain*, int, int32_t*, int, int*, int*) = cvs_contour_chains_batch;\n'
                'int (*refine)(cvs_handle, int, int, const cvs_plane*, const cvs_plane*, const int32_t*, int, const int32_t*, float*, float*, int)'
                ' = cvs_chain_refine_batch;\n'
                'int main() { return chains == 0 || refine == 0; }\n')
    subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), src], check=True)


def test_library_exports_and_binds():
    import cvsteer_amd
    from cvsteer_amd import _lib as L
    assert L.SIGNATURES["cvs_contour_chains_batch"] == (C.c_int, [C.c_void_p, C.c_int, L._PP, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                                  C.c_int, L._IP, L._IP])
    assert L.SIGNATURES["cvs_chain_refine_batch"] == (C.c_int, [C.c_void_p, C.c_int, C.c_int, L._PP, L._PP, C.c_void_p, C.c_int, C.c_void_p,
                                                                C.c_void_p, C.c_void_p, C.c_int])
    hip = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "cvsteer_amd", "libcvsteer_hip.so")], text=True)
    for name in NAMES:
        assert re.search(r" T %s$" % name, hip, re.M), name
    # the sanitizer twin and the canary twins of the library link the units of these two lists: the new units are in them
    make = open(os.path.join(SRC, "Makefile")).read()
    assert re.search(r"^HOST_UNITS\s*=.*\bcvs_chains_batch\b", make, re.M) and re.search(r"^KERNEL_UNITS\s*=.*\bcvs_kernels_chains_batch\b", make, re.M)
    for cls in (cvsteer_amd.SteerableFiltersG2, cvsteer_amd.SteerableFiltersG4):
        for name in ("contour_chains_batch", "chain_refine_batch", "contour_edgels_batch"):
            assert callable(getattr(cls, name, None)), name


def test_null_handle():
    from cvsteer_amd import _lib as L
    img = np.zeros((4, 4), np.float32)
    plane = L.Plane(img.ctypes.data, 4, 4, 16, L.MEM_HOST)
    pts, tab, rng = np.full((8, 2), -9, np.int32), np.full((4, 4), -9, np.int32), np.full((2, 2), -9, np.int32)
    xy, st = np.full((8, 2), -9, np.float32), np.full((8,), -9, np.float32)
    n, m = C.c_int(-5), C.c_int(-6)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert L.lib().cvs_contour_chains_batch(None, 1, C.byref(plane), p(pts), 8, p(tab), 4, p(rng), L.MEM_HOST, C.byref(n), C.byref(m)) == L.E_BADARG
    assert L.lib().cvs_chain_refine_batch(None, 1, 1, C.byref(plane), C.byref(plane), p(pts), 8, p(rng), p(xy), p(st), L.MEM_HOST) == L.E_BADARG
    assert (n.value, m.value) == (-5, -6)
    assert all((a == -9).all() for a in (pts, tab, rng, xy, st))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_batch_kernels_use_no_scratch(tmp_path):
    path = os.path.join(str(tmp_path), "cvs_kernels_chains_batch.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    "-I" + SRC, "-S", "--cuda-device-only", os.path.join(SRC, "cvs_kernels_chains_batch.hip"), "-o", path], check=True,
                   stderr=subprocess.DEVNULL)
    text = open(path).read()
    scratch = {}
    for blk in text.split("  - .agpr_count:")[1:]:
        nm = re.search(r"\.name:\s+(\S+)", blk)
        ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        if nm and ps:
            scratch[nm.group(1)] = int(ps.group(1))
    stems = ("k_chb_table", "k_chb_links", "k_chb_tiles", "k_chb_borders", "k_chb_head_apply", "k_chb_emit", "k_chb_ranges", "k_chain_refine_batch")
    for stem in stems:
        assert any(stem in n for n in scratch), (stem, sorted(scratch))
    assert len(scratch) == len(stems) and all(v == 0 for v in scratch.values()), scratch
    # the point and the position travel as one 8-byte access each, as in k_chain_refine
    body = text[text.index("k_chain_refine_batch"):]
    body = body[:body.index(".Lfunc_end")]
    assert "global_load_dwordx2" in body and "global_store_dwordx2" in body


def test_the_units_the_issue_keeps_are_untouched():
    """the batch path is new files around the old launches: the kernel counts of the single-image units are pinned by their own tests, and the
    new host unit includes their descriptors rather than copies of them"""
    host = open(os.path.join(SRC, "cvs_chains_batch.cpp")).read()
    for call in ("launch_ch_nodes", "launch_ch_roots", "launch_ch_arc_count", "launch_ch_arc_base", "launch_ch_arcs", "launch_ch_jump",
                 "launch_ch_heads", "launch_ch_head_count", "launch_scan_partials"):
        assert call + "(" in host, call


# ---- the model: per-plane chains concatenated == one run on the stacked planes ----
def _planes(rng, shape, density, n, empty=()):
    out = [(rng.random(shape) < density).astype(np.float32) for _ in range(n)]
    for z in empty:
        out[z][:] = 0
    return out


def _same(a, b):
    return all(x.dtype == np.int32 and y.dtype == np.int32 and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("shape", [(7, 9), (33, 65)])
def test_concatenation_is_the_stacked_reading(shape):
    rng = np.random.default_rng(shape[0])
    chains = 0
    for density in (0.1, 0.3, 0.6):
        for n, empty in ((1, ()), (2, ()), (5, ()), (5, (0,)), (5, (2,)), (5, (4,)), (5, (0, 1, 4)), (2, (0, 1))):
            masks = _planes(rng, shape, density, n, empty)
            got, want = M.chains_batch(masks), M.stacked(masks)
            assert _same(got, want), (density, n, empty)
            pts, table, ranges = got
            assert ranges.shape == (n + 1, 2) and ranges[0].tolist() == [0, 0] and ranges[n].tolist() == [len(table), len(pts)]
            assert (np.diff(ranges, axis=0) >= 0).all()
            for z in range(n):
                c0, c1 = ranges[z, 0], ranges[z + 1, 0]
                assert (table[c0:c1, 3] == z).all()
                p, t = CM.chains(masks[z])
                assert np.array_equal(pts[ranges[z, 1]:ranges[z + 1, 1]], p)
                assert np.array_equal(table[c0:c1, 1:3], t[:, 1:3]) and np.array_equal(table[c0:c1, 0] - ranges[z, 1], t[:, 0])
            for z in empty:
                assert ranges[z].tolist() == ranges[z + 1].tolist()             # an empty plane repeats its successor's pair
            chains += len(table)
    assert chains > 100


def test_hand_case_two_planes():
    a = np.float32([[1, 1, 1], [0, 0, 0], [0, 1, 0]])                             # a bar, and a pixel in the last row
    b = np.float32([[0, 1, 1], [0, 0, 0], [0, 0, 0]])                             # straight and diagonally below it, in row 0 of the next plane
    pts, table, ranges = M.chains_batch([a, b])
    assert table.tolist() == [[0, 3, 0, 0], [3, 1, 0, 0], [4, 2, 0, 1]]
    assert pts.tolist() == [[0, 0], [1, 0], [2, 0], [1, 2], [1, 0], [2, 0]]
    assert ranges.tolist() == [[0, 0], [2, 4], [3, 6]]
    assert _same((pts, table, ranges), M.stacked([a, b]))
