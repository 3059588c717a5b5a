"""Contour segments (cvs_polyline_segments) at every layer that exists without a GPU: the public header, the exports of both libraries,
the Python surface, the generated code of the new kernels (no scratch), and the model of segments_model.py that the GPU tests hold the
kernels against -- hand cases with known answers, the derived sequence against numpy.linalg.eigh, and the geometry of straight ridges:
what the fit on the sub-pixel points gains over the chord of the integer polyline and over a fit on the pixel centres."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import chains_model as CM
import contour_model as NM
import polyline_model as PM
import refine_model as RM
import segments_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "cvsteer_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
F32 = np.float32
OFFSETS = dict(first=0, count=4, chain=8, flags=12, w=16, sx=24, sy=32, sxx=40, sxy=48, syy=56, cx=64, cy=72, ux=80, uy=88, t0=96, t1=104,
               rms=112, dmax=120)


# ---- header, binding and build ----
def test_header_declares_the_call_and_the_record(tmp_path):
    text = open(os.path.join(ROOT, "include", "cvsteer_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int cvs_polyline_segments\(cvs_handle h,\s*const int32_t\* points, int n_points,\s*const cvs_chain\* chains, "
                     r"const cvs_chain\* polylines, int n_chains,\s*const int32_t\* index, int n_vertices,\s*const float\* xy,\s*"
                     r"const float\* strength,\s*cvs_segment\* table,\s*int mem\);", plain)
    assert re.search(r"#define CVS_ABI_VERSION 2\b", text)
    src = os.path.join(str(tmp_path), "use.cpp")
    with open(src, "w") as f:
        f.write('#include <stddef.h>\n#include "cvsteer_hip.h"\n'
                'static_assert(sizeof(cvs_segment) == 128 && CVS_SEG_WRAPS == 1 && CVS_SEG_DEGENERATE == 2, "128 bytes, two flags");\n'
                + "".join('static_assert(offsetof(cvs_segment, %s) == %d, "%s");\n' % (n, o, n) for n, o in OFFSETS.items()) +
                'int (*fit)(cvs_handle, const int32_t*, int, const cvs_chain*, const cvs_chain*, int, const int32_t*, int, const float*,'
                ' const float*, cvs_segment*, int) = cvs_polyline_segments;\n'
                'int main() { return fit == 0; }\n')
    subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), src], check=True)


def test_libraries_export_and_bind():
    import cvsteer_amd
    from cvsteer_amd import _lib as L
    assert L.SIGNATURES["cvs_polyline_segments"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                               C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int])
    assert C.sizeof(L.Segment) == 128 == M.SEGMENT_DTYPE.itemsize
    assert (L.SEG_WRAPS, L.SEG_DEGENERATE) == (M.WRAPS, M.DEGENERATE) == (cvsteer_amd.SEG_WRAPS, cvsteer_amd.SEG_DEGENERATE)
    hip = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "cvsteer_amd", "libcvsteer_hip.so")], text=True)
    assert re.search(r" T cvs_polyline_segments$", hip, re.M)
    so = os.path.join(ROOT, "cvsteer_amd", "libcvsteer.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cvsteer_amd", "facade"), "-s"])
    syms = subprocess.check_output(["nm", "-DC", "--defined-only", so], text=True)
    for cls in ("SteerableFiltersG2", "SteerableFiltersG4"):
        assert re.search(r" T fa::%s::fitSegments\(fa::Mat1f const&, std::vector<std::vector<fa::Point," % cls, syms), cls
    for cls in (cvsteer_amd.SteerableFiltersG2, cvsteer_amd.SteerableFiltersG4):
        assert all(callable(getattr(cls, name, None)) for name in ("polyline_segments", "contour_segments"))
        assert cls.SEGMENT_DTYPE == M.SEGMENT_DTYPE
        assert {n: cls.SEGMENT_DTYPE.fields[n][1] for n in cls.SEGMENT_DTYPE.names} == OFFSETS
        assert [(n, getattr(L.Segment, n).offset) for n, _ in L.Segment._fields_] == list(OFFSETS.items())


def test_null_handle():
    from cvsteer_amd import _lib as L
    pts = np.int32([[0, 0], [1, 0], [2, 0]])
    tab, pol, idx = np.int32([[0, 3, 0, 0]]), np.int32([[0, 2, 0, 0]]), np.int32([0, 2])
    rec = np.full((2, 32), -9, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert L.lib().cvs_polyline_segments(None, p(pts), 3, p(tab), p(pol), 1, p(idx), 2, None, None, p(rec), L.MEM_HOST) == L.E_BADARG
    assert (rec == -9).all()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_segment_kernels_use_no_scratch(tmp_path):
    path = os.path.join(str(tmp_path), "cvs_kernels_segments.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    "-I" + SRC, "-S", "--cuda-device-only", os.path.join(SRC, "cvs_kernels_segments.hip"), "-o", path], check=True,
                   stderr=subprocess.DEVNULL)
    text = open(path).read()
    scratch = {}
    for blk in text.split("  - .agpr_count:")[1:]:
        nm = re.search(r"\.name:\s+(\S+)", blk)
        ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        if nm and ps:
            scratch[nm.group(1)] = int(ps.group(1))
    for stem in ("k_segments_wave", "k_segments_block"):
        assert any(stem in n for n in scratch), (stem, sorted(scratch))
    assert len(scratch) == 2 and all(v == 0 for v in scratch.values()), scratch


# ---- the model on its own: hand cases ----
def _one(points, flags=0, index=None, xy=None, strength=None):
    """the records of ONE chain that holds all `points`, its polyline vertices at `index` (default: the two ends)"""
    points = np.asarray(points, np.int32).reshape(-1, 2)
    index = np.int32([0, len(points) - 1] if index is None else index)
    return M.segments(points, np.int32([[0, len(points), flags, 0]]), np.int32([[0, len(index), flags, 0]]), index, xy=xy, strength=strength)


def test_model_a_horizontal_run_of_five_points():
    seg = _one([(3, 7), (4, 7), (5, 7), (6, 7), (7, 7)])
    a, last = seg[0], seg[1]
    assert (a["first"], a["count"], a["chain"], a["flags"]) == (0, 5, 0, 0)
    assert [a[n] for n in M.SUMS] == [5.0, 10.0, 0.0, 30.0, 0.0, 0.0]          # offsets 0 .. 4 from the first pixel
    assert (a["cx"], a["cy"], a["ux"], a["uy"], a["t0"], a["t1"], a["rms"], a["dmax"]) == (5.0, 7.0, 1.0, 0.0, -2.0, 2.0, 0.0, 0.0)
    assert last.tobytes() == np.array([(4, 0, 0, 0) + (0.0,) * 14], M.SEGMENT_DTYPE).tobytes()   # the last vertex of an open polyline: no span
    assert M.end_points(seg[:1]).tolist() == [[3.0, 7.0, 7.0, 7.0]]
    back = _one([(7, 7), (6, 7), (5, 7), (4, 7), (3, 7)])[0]                    # the direction runs from the first point to the last
    assert (back["ux"], back["uy"], back["t0"], back["t1"], back["cx"]) == (-1.0, 0.0, -2.0, 2.0, 5.0)


def test_model_a_three_four_five_diagonal():
    seg = _one([(0, 0), (4, 3), (8, 6)])[0]
    assert (seg["count"], seg["flags"]) == (3, 0) and (seg["cx"], seg["cy"]) == (4.0, 3.0)
    assert abs(seg["ux"] - 0.8) < 1e-15 and abs(seg["uy"] - 0.6) < 1e-15 and abs(seg["t0"] + 5.0) < 1e-14 and abs(seg["t1"] - 5.0) < 1e-14
    assert seg["rms"] < 1e-7 and seg["dmax"] < 1e-14
    # the middle point 0.625 px off along the normal (-0.6, 0.8): the direction stays, the line moves a third of the way, and the points lie
    # 0.625 / 3, 2 * 0.625 / 3 and 0.625 / 3 from it
    off = _one([(0, 0), (4, 3), (8, 6)], xy=F32([[0, 0], [4 - 0.375, 3 + 0.5], [8, 6]]))[0]
    assert abs(off["ux"] - 0.8) < 1e-12 and abs(off["dmax"] - 2 * 0.625 / 3) < 1e-12 and abs(off["rms"] - 0.625 * np.sqrt(2.0) / 3) < 1e-12


def test_model_two_points_and_degenerate_spans():
    seg = _one([(2, 9), (2, 5)])[0]                                            # straight up: ux == 0, the direction from first to last
    assert (seg["count"], seg["ux"], seg["uy"], seg["t0"], seg["t1"], seg["cx"], seg["cy"], seg["rms"], seg["dmax"]) == \
           (2, 0.0, -1.0, -2.0, 2.0, 2.0, 7.0, 0.0, 0.0)
    same = _one([(4, 4), (9, 9), (4, 4)], xy=F32([[1, 1], [1, 1], [1, 1]]))[0]   # all positions equal: no direction
    assert same["flags"] == M.DEGENERATE and (same["cx"], same["cy"]) == (1.0, 1.0) and same["w"] == 3.0
    assert all(np.isnan(same[n]) for n in ("ux", "uy", "t0", "t1", "rms", "dmax"))
    nan = _one([(0, 0), (1, 0), (2, 0)], xy=F32([[0, 0], [np.nan, 0], [2, 0]]), strength=F32([1, -1, 1]))[0]
    assert nan["flags"] == M.DEGENERATE and np.isnan(nan["sx"]) and nan["w"] == 2.0 and np.isnan(nan["cx"]) and nan["cy"] == 0.0
    assert all(np.isnan(nan[n]) for n in ("ux", "uy", "t0", "t1", "rms", "dmax"))     # a NaN position counts whatever its weight


def test_model_a_closed_ring_with_one_vertex():
    ring = [(0, 0), (1, 0), (2, 0), (2, 1), (2, 2), (1, 2), (0, 2), (0, 1)]
    seg = _one(ring, flags=CM.CLOSED, index=[0])
    assert len(seg) == 1 and (seg[0]["first"], seg[0]["count"], seg[0]["flags"] & M.WRAPS) == (0, 9, M.WRAPS)   # the cycle, its start twice
    sp = M.spans(np.int32([[0, 8, 1, 0]]), np.int32([[0, 1, 1, 0]]), np.int32([0]))
    assert sp[0][4].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 0]
    assert seg[0]["w"] == 9.0 and (seg[0]["sx"], seg[0]["sy"]) == (8.0, 8.0)
    # three vertices: two inner spans and the span that wraps, each vertex in both of its spans
    sp = M.spans(np.int32([[0, 8, 1, 0]]), np.int32([[0, 3, 1, 0]]), np.int32([1, 4, 6]))
    assert [s[4].tolist() for s in sp] == [[1, 2, 3, 4], [4, 5, 6], [6, 7, 0, 1]] and [s[3] for s in sp] == [0, 0, M.WRAPS]
    # the same ring open: its last vertex has no span; a polyline of length 0 is skipped by the search
    sp = M.spans(np.int32([[0, 3, 0, 0], [3, 1, 0, 0], [4, 4, 0, 0]]), np.int32([[0, 2, 0, 0], [2, 0, 0, 0], [2, 2, 0, 0]]), np.int32([0, 2, 4, 7]))
    assert [(s[1], s[2]) for s in sp] == [(3, 0), (0, 0), (4, 2), (0, 2)]


def test_model_weights():
    pts = [(0, 0), (1, 0), (2, 7), (3, 1), (4, 3)]                             # (the third point lies far from any line through the others)
    xy = (np.array(pts) + [[0.25, -0.125]] * 5).astype(F32)
    unit = _one(pts, xy=xy)[0]
    ones = _one(pts, xy=xy, strength=F32([1, 1, 1, 1, 1]))[0]
    assert unit.tobytes() == ones.tobytes()
    st = F32([2.0, np.nan, -3.0, 0.5, 1.0])                                     # NaN and a negative strength weigh 0
    got = _one(pts, xy=xy, strength=st)[0]
    want = _one([pts[0], pts[3], pts[4]], xy=xy[[0, 3, 4]], strength=st[[0, 3, 4]])[0]
    assert got["w"] == 3.5 and all(got[n] == want[n] for n in M.SUMS + ("cx", "cy", "ux", "uy", "t0", "t1", "rms"))
    assert got["count"] == 5 and got["dmax"] > want["dmax"] > 0                # ... but every point counts for dmax
    zero = _one(pts, xy=xy, strength=F32([0, -1, np.nan, 0, -0.0]))[0]
    assert zero["flags"] == M.DEGENERATE and zero["w"] == 0.0 and np.isnan(zero["cx"]) and np.isnan(zero["cy"]) and np.isnan(zero["dmax"])
    assert [zero[n] for n in M.SUMS] == [0.0] * 6


def test_model_orientation_ties():
    # a span that comes back to where it started: q = 0, so s == 0 and the sign of (ux, uy) decides: ux > 0, or ux == 0 and uy > 0
    for pts, want in (([(0, 0), (3, 0), (6, 0), (3, 0), (0, 0)], (1.0, 0.0)), ([(0, 0), (0, 2), (0, 5), (0, 2), (0, 0)], (0.0, 1.0)),
                      ([(5, 5), (3, 7), (1, 9), (3, 7), (5, 5)], (np.sqrt(0.5), -np.sqrt(0.5)))):
        seg = _one(pts)[0]
        assert seg["flags"] == 0 and abs(seg["ux"] - want[0]) < 1e-15 and abs(seg["uy"] - want[1]) < 1e-15, (pts, seg)
        assert seg["t0"] == seg["t1"]
    line = M.derive([2.0, 0.0, 2.0, 0.0, 0.0, 4.0], (0.0, 0.0), (0.0, 0.0), (0, 0))      # the raw eigenvector is (0, +) already
    assert (line["ux"], line["uy"]) == (0.0, 1.0) and not np.signbit(line["ux"])
    line = M.derive([2.0, 0.0, 2.0, 0.0, 0.0, 4.0], (0.0, 2.0), (0.0, 0.0), (0, 0))      # s < 0 turns it round
    assert (line["ux"], line["uy"]) == (0.0, -1.0)


def test_derive_against_eigh():
    rng = np.random.default_rng(17)
    worst_dir = worst_val = 0.0
    for trial in range(200):
        n = int(rng.integers(3, 60))
        ang = rng.uniform(0, np.pi)
        along = np.sort(rng.uniform(0, 40, n))
        across = rng.normal(0, rng.choice([0.01, 0.3, 3.0]), n)
        p = np.stack([along * np.cos(ang) - across * np.sin(ang), along * np.sin(ang) + across * np.cos(ang)], axis=1) + rng.uniform(-50, 50, 2)
        xy = p.astype(F32)
        pts = np.rint(xy).astype(np.int32)
        st = rng.uniform(0.1, 2.0, n).astype(F32) if trial % 2 else None
        seg = _one(pts, xy=xy, strength=st)[0]
        w = np.ones(n) if st is None else st.astype(np.float64)
        q = xy.astype(np.float64)
        mean = (w[:, None] * q).sum(0) / w.sum()
        d = q - mean
        cov = (w[:, None, None] * d[:, :, None] * d[:, None, :]).sum(0)
        val, vec = np.linalg.eigh(cov)
        major = vec[:, 1]
        cross = abs(seg["ux"] * major[1] - seg["uy"] * major[0])              # sin of the angle between the two, up to sign
        worst_dir = max(worst_dir, float(np.arcsin(min(cross, 1.0))))
        worst_val = max(worst_val, abs(seg["rms"] ** 2 * seg["w"] - val[0]) / (val[0] + val[1]))
        assert abs(seg["cx"] - mean[0]) < 1e-10 and abs(seg["cy"] - mean[1]) < 1e-10
        assert seg["ux"] * (q[-1, 0] - q[0, 0]) + seg["uy"] * (q[-1, 1] - q[0, 1]) >= 0
        assert abs(seg["dmax"] - np.abs(major[0] * d[:, 1] - major[1] * d[:, 0]).max()) < 1e-8
    print("derive against eigh, 200 spans: direction within %.3g rad, smaller eigenvalue within %.3g of the trace" % (worst_dir, worst_val))
    assert worst_dir <= 1e-9 and worst_val <= 1e-9


def test_exact_sums_round_once_and_bound_any_order():
    rng = np.random.default_rng(3)
    pts = np.cumsum(rng.integers(0, 2, (400, 2)), axis=0).astype(np.int32)
    xy = (pts + rng.uniform(-0.5, 0.5, pts.shape)).astype(F32)
    st = rng.standard_normal(400).astype(F32)
    tab, pol, idx = np.int32([[0, 400, 0, 0]]), np.int32([[0, 3, 0, 0]]), np.int32([0, 150, 399])
    ex = M.exact_sums(pts, tab, pol, idx, xy, st)
    assert ex[2] == (None, None)
    for (first, count, _, _, pos), (sums, mags) in zip(M.spans(tab, pol, idx)[:2], ex[:2]):
        t = M.terms(pts, xy, st, first, pos)
        for order in (np.arange(count), np.arange(count)[::-1], rng.permutation(count)):
            for row, s, m in zip(t, sums, mags):
                acc = np.float64(0.0)
                for v in row[order]:
                    acc = acc + v
                assert abs(float(acc) - s) <= (count + 2) * 2.0 ** -52 * m


# ---- the geometry table ----
def _angle_error(ux, uy, deg):
    return abs((np.rad2deg(np.arctan2(uy, ux)) - deg + 90.0) % 180.0 - 90.0)


def test_ridge_segments_geometry_table():
    """The 13 ridges of refine_model (48 x 48, GEOMETRY_ANGLES), the selection of test_ridges_are_located_to_a_tenth_of_a_pixel, then
    chains_model.chains -> polyline_model.polylines(eps = 1.0) -> the fit of every span of >= 8 points.  Worst figures over the 15 spans,
    measured on a CPU: the chord between the two integer vertices 5.814 degrees and 0.6905 px (a vertex off the true line); the fit on the
    pixel centres 2.682 degrees and 0.3000 px; the fit on the sub-pixel points 0.1182 degrees and 0.02089 px (the centroid off the line)."""
    worst = {"chord": [0.0, 0.0], "pixel centres": [0.0, 0.0], "sub-pixel": [0.0, 0.0]}
    n_spans = 0
    for deg in RM.GEOMETRY_ANGLES:
        img, theta, dist = RM.ridge(48, deg)
        c, s = RM.directions(theta)
        P = RM.refine_map(img, c, s)
        sel = NM.nonmax_parts(img, c, s)[0] > 0.5
        sel[:6], sel[-6:], sel[:, :6], sel[:, -6:] = False, False, False, False
        pts, chains = CM.chains(sel.astype(F32))
        _, pol, idx = PM.polylines(pts, chains, 1.0)
        xy, _ = RM.gather(P, pts)
        fit, pix = M.segments(pts, chains, pol, idx, xy=xy), M.segments(pts, chains, pol, idx)
        for f, p in zip(fit, pix):
            if f["count"] < 8:
                continue
            assert not f["flags"]
            n_spans += 1
            a, b = pts[f["first"]].astype(np.float64), pts[f["first"] + f["count"] - 1].astype(np.float64)
            for name, ang, off in (("chord", _angle_error(b[0] - a[0], b[1] - a[1], deg), max(abs(dist(*a)), abs(dist(*b)))),
                                   ("pixel centres", _angle_error(p["ux"], p["uy"], deg), abs(dist(p["cx"], p["cy"]))),
                                   ("sub-pixel", _angle_error(f["ux"], f["uy"], deg), abs(dist(f["cx"], f["cy"])))):
                worst[name] = [max(worst[name][0], float(ang)), max(worst[name][1], float(off))]
    print("straight segments of 13 ridges, %d spans of >= 8 points: worst angle error / distance of the anchor from the true line" % n_spans)
    for name, (ang, off) in worst.items():
        print("  %-14s %7.4f deg  %7.4f px" % (name, ang, off))
    assert n_spans >= 13
    assert worst["sub-pixel"][0] <= 0.2 and worst["sub-pixel"][1] <= 0.03
    assert worst["chord"][0] > 5.0 and worst["chord"][1] > 0.6
    assert worst["sub-pixel"][0] < worst["pixel centres"][0] < worst["chord"][0]
