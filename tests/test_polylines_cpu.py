"""Contour polylines (cvs_chain_polylines) at every layer that exists without a GPU: the public header, the exports of both libraries, the
Python surface, the generated code of the new kernels (no scratch), and the Python model the GPU tests hold the kernels against -- its own
invariants on the chains of random masks, and hand cases with the expected lists written out."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import chains_model as CM
import polyline_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "cvsteer_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
INF = float("inf")


def test_header_declares_the_call_and_reuses_cvs_chain(tmp_path):
    text = open(os.path.join(ROOT, "include", "cvsteer_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int cvs_chain_polylines\(cvs_handle h,\s*const int32_t\* points, int n_points,\s*const cvs_chain\* chains, int n_chains,\s*"
                     r"float eps,\s*int32_t\* vertices, int vertex_capacity,\s*int32_t\* index,\s*cvs_chain\* polylines,\s*int mem,\s*"
                     r"int\* n_vertices\);", plain)
    assert re.search(r"#define CVS_ABI_VERSION 2\b", text)
    assert len(re.findall(r"typedef struct cvs_chain\b", text)) == 1          # the table of the polylines is the chains' own struct
    src = os.path.join(str(tmp_path), "use.cpp")
    with open(src, "w") as f:
        f.write('#include <stddef.h>\n#include "cvsteer_hip.h"\n'
                'static_assert(sizeof(cvs_chain) == 16, "16 bytes");\n'
                'int (*call)(cvs_handle, const int32_t*, int, const cvs_chain*, int, float, int32_t*, int, int32_t*, cvs_chain*, int, int*)'
                ' = cvs_chain_polylines;\n'
                'int main() { return call == 0; }\n')
    subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), src], check=True)
    hdr = open(os.path.join(SRC, "cvs_polyline.h")).read()
    t = int(re.search(r"constexpr int kPlWaveMax = (\d+);", hdr).group(1))
    assert 64 < t <= 1024


def test_libraries_export_and_bind():
    import cvsteer_amd
    from cvsteer_amd import _lib as L
    assert L.SIGNATURES["cvs_chain_polylines"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_void_p,
                                                             C.c_int, C.c_void_p, C.c_void_p, C.c_int, L._IP])
    assert M.CLOSED == cvsteer_amd.CHAIN_CLOSED == 1
    hip = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "cvsteer_amd", "libcvsteer_hip.so")], text=True)
    assert re.search(r" T cvs_chain_polylines$", hip, re.M)
    so = os.path.join(ROOT, "cvsteer_amd", "libcvsteer.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cvsteer_amd", "facade"), "-s"])
    syms = subprocess.check_output(["nm", "-DC", "--defined-only", so], text=True)
    for cls in ("SteerableFiltersG2", "SteerableFiltersG4"):
        assert re.search(r" T fa::%s::approxContours\(std::vector<std::vector<fa::Point," % cls, syms), cls
    for cls in (cvsteer_amd.SteerableFiltersG2, cvsteer_amd.SteerableFiltersG4):
        assert callable(getattr(cls, "chain_polylines", None)) and callable(getattr(cls, "contour_polylines", None))


def test_null_handle():
    from cvsteer_amd import _lib as L
    pts = np.zeros((3, 2), np.int32)
    tab = np.array([[0, 3, 0, 0]], np.int32)
    out, pol = np.full((3, 2), -9, np.int32), np.full((1, 4), -9, np.int32)
    v = C.c_int(-5)
    rc = L.lib().cvs_chain_polylines(None, C.c_void_p(pts.ctypes.data), 3, C.c_void_p(tab.ctypes.data), 1, 1.0, C.c_void_p(out.ctypes.data), 3,
                                     None, C.c_void_p(pol.ctypes.data), L.MEM_HOST, C.byref(v))
    assert rc == L.E_BADARG and v.value == -5 and (out == -9).all() and (pol == -9).all()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_polyline_kernels_use_no_scratch(tmp_path):
    path = os.path.join(str(tmp_path), "cvs_kernels_polyline.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    "-I" + SRC, "-S", "--cuda-device-only", os.path.join(SRC, "cvs_kernels_polyline.hip"), "-o", path], check=True,
                   stderr=subprocess.DEVNULL)
    text = open(path).read()
    scratch = {}
    for blk in text.split("  - .agpr_count:")[1:]:
        nm = re.search(r"\.name:\s+(\S+)", blk)
        ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        if nm and ps:
            scratch[nm.group(1)] = int(ps.group(1))
    for stem in ("k_pl_keep_wave", "k_pl_keep_block", "k_pl_count", "k_pl_apply", "k_pl_emit_wave", "k_pl_emit_block"):
        assert any(stem in n for n in scratch), (stem, sorted(scratch))
    assert len(scratch) == 6 and all(v == 0 for v in scratch.values()), scratch


# ---- the model against the contract's own consequences ----
def _check_chain(pts, flags, eps):
    """the invariants of one chain; returns its kept indices"""
    closed = bool(flags & M.CLOSED)
    keep = M.kept(pts, closed, eps)
    L = len(pts)
    assert keep == sorted(set(keep)) and all(0 <= i < L for i in keep)
    assert keep[0] == 0 and (closed or keep[-1] == L - 1)                      # the end points are kept
    if L <= 2:
        assert keep == list(range(L))
        return keep
    q = M.virtual_list(pts, closed)
    kq = keep + ([L] if closed else [])                                       # kept indices of the virtual list
    for lo, hi in zip(kq[:-1], kq[1:]):
        # every dropped point passes the "not greater" test against the segment that covers it ...
        for i in range(lo + 1, hi):
            assert not M.splits(M.value(q[lo], q[hi], q[i]), q[lo], q[hi], eps)
        # ... and that segment, run through the model again as an open chain of its own, keeps its two ends only
        if hi - lo >= 2:
            assert M.kept(q[lo:hi + 1], False, eps) == [0, hi - lo]
    # the first split divides the problem: the kept set is that of the two halves, whichever is visited first
    if len(q) > 2:
        m, v = M.split_point(q, 0, len(q) - 1)
        if M.splits(v, q[0], q[-1], eps) and m >= 2 and len(q) - 1 - m >= 2:
            left, right = M.kept(q[:m + 1], False, eps), M.kept(q[m:], False, eps)
            assert sorted(set(left) | {m + i for i in right}) == kq
    if eps == INF and not closed and q[0] != q[-1]:
        assert keep == [0, L - 1]
    return keep


def test_model_invariants_on_the_chains_of_random_masks():
    rng = np.random.default_rng(77)
    n_chains, n_long = 0, 0
    for density in (0.15, 0.3, 0.5):
        for _ in range(4):
            shape = tuple(int(v) for v in rng.integers(12, 30, 2))
            mask = (rng.random(shape) < density).astype(np.float32)
            pts, table = CM.chains(mask)
            prev = None
            for eps in (0.0, 0.5, 1.0, 1.5, INF):
                vtx, pol, idx = M.polylines(pts, table, eps)
                assert vtx.dtype == np.int32 and pol.dtype == np.int32 and idx.dtype == np.int32
                assert np.array_equal(vtx, pts[idx]) and len(vtx) <= len(pts)
                assert pol[:, 0].tolist() == np.concatenate([[0], np.cumsum(pol[:, 1])[:-1]]).astype(int).tolist()
                assert np.array_equal(pol[:, 2], table[:, 2]) and (pol[:, 3] == 0).all()
                for (s, n, f, _), (ps, pn, _, _) in zip(table.tolist(), pol.tolist()):
                    keep = _check_chain(pts[s:s + n].tolist(), f, eps)
                    assert [s + i for i in keep] == idx[ps:ps + pn].tolist()
                    n_long += n > 2
                if eps == 0.0:
                    assert len(vtx) <= len(pts)
                prev = len(vtx)
            n_chains += len(table)
            assert prev is not None
    assert n_chains >= 200 and n_long >= 200, (n_chains, n_long)


# ---- hand cases, the expected lists written out ----
def _kept(pts, eps, closed=False):
    return M.kept([tuple(p) for p in pts], closed, eps)


def test_straight_run_keeps_its_ends_also_at_eps_zero():
    run = [(x, 0) for x in range(5)]
    assert _kept(run, 1.0) == [0, 4]
    assert _kept(run, 0.0) == [0, 4]          # the distance is 0 and the test is strict
    assert _kept([(x, x) for x in range(5)], 0.0) == [0, 4]


TENT = [(0, 2), (0, 1), (0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (4, 1), (4, 2)]


def test_tent_at_the_tolerance_and_just_below_it():
    assert _kept(TENT, 2.0) == [0, 8]         # the distance is exactly 2: not greater
    below = float(np.nextafter(np.float32(2.0), np.float32(0.0)))
    assert _kept(TENT, below) == [0, 2, 8]    # five points tie at distance 2, the smallest index wins; (0,0) -> (4,2) then holds the rest
    assert _kept(TENT, 0.0) == [0, 2, 6, 8]
    vtx, pol, idx = M.polylines(np.int32(TENT), np.int32([[0, 9, 0, 0]]), below)
    assert vtx.tolist() == [[0, 2], [0, 0], [4, 2]] and pol.tolist() == [[0, 3, 0, 0]] and idx.tolist() == [0, 2, 8]


RING = [(0, 0), (1, 0), (2, 0), (3, 0), (3, 1), (3, 2), (3, 3), (2, 3), (1, 3), (0, 3), (0, 2), (0, 1)]


def test_closed_ring_keeps_its_corners():
    m = np.zeros((4, 4), np.float32)
    m[0, :] = m[3, :] = m[:, 0] = m[:, 3] = 1
    pts, table = CM.chains(m)
    assert pts.tolist() == [list(p) for p in RING] and table.tolist() == [[0, 12, CM.CLOSED, 0]]
    assert _kept(RING, 1.0, closed=True) == [0, 3, 6, 9]      # a == b: the farthest point first, then the two diagonals split at the corners
    assert _kept(RING, 0.0, closed=True) == [0, 3, 6, 9]
    assert _kept(RING, INF, closed=True) == [0]               # the repeated first point is virtual
    assert _kept(RING, 1.0, closed=False) == [0, 3, 6, 9, 11]
    vtx, pol, idx = M.polylines(pts, table, 1.0)
    assert vtx.tolist() == [[0, 0], [3, 0], [3, 3], [0, 3]] and pol.tolist() == [[0, 4, CM.CLOSED, 0]]


def test_ring_with_a_tail_is_an_open_chain_with_equal_ends():
    loop = [(2, 2), (3, 2), (4, 2), (4, 3), (4, 4), (3, 4), (2, 4), (2, 3), (2, 2)]
    assert _kept(loop, 1.0) == [0, 2, 4, 6, 8]
    assert _kept(loop, INF) == [0, 8]
    assert _kept(loop, 3.0) == [0, 8]          # the farthest point is sqrt(8) away
    m = np.zeros((6, 6), np.float32)           # the same loop hung on a tail: the model of the chains lists it so
    m[2, 0:5] = m[4, 2:5] = m[2:5, 2] = m[2:5, 4] = 1
    pts, table = CM.chains(m)
    loops = [(s, n, f) for s, n, f, _ in table.tolist() if n > 2 and pts[s].tolist() == pts[s + n - 1].tolist()]
    assert len(loops) == 1 and not loops[0][2] & CM.CLOSED
    s, n, f = loops[0]
    k = M.kept(pts[s:s + n].tolist(), False, 1.0)
    assert k[0] == 0 and k[-1] == n - 1 and len(k) == 5


def test_isolated_point_and_two_point_chain():
    for eps in (0.0, 1.0, INF):
        assert _kept([(5, 7)], eps) == [0]
        assert _kept([(5, 7), (6, 8)], eps) == [0, 1]
        assert _kept([(5, 7), (6, 8)], eps, closed=True) == [0, 1]   # L <= 2: every point is kept
    vtx, pol, idx = M.polylines(np.int32([[5, 7], [1, 1], [2, 2]]), np.int32([[0, 1, 0, 0], [1, 2, 0, 0]]), INF)
    assert vtx.tolist() == [[5, 7], [1, 1], [2, 2]] and pol.tolist() == [[0, 1, 0, 0], [1, 2, 0, 0]] and idx.tolist() == [0, 1, 2]
    vtx, pol, idx = M.polylines(np.zeros((0, 2), np.int32), np.zeros((0, 4), np.int32), 1.0)
    assert vtx.shape == (0, 2) and pol.shape == (0, 4) and idx.shape == (0,)
