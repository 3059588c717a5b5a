"""Contour turns (cvs_chain_turns) at every layer that exists without a GPU: the public header, the exports of both libraries, the Python
surface, the generated code of the new kernels (no scratch; the host table check runs under the host sanitizers in test_joins_cpu.py), and
the model of turns_model.py that the GPU tests hold the kernels against -- hand cases with known answers, and the geometry of digital
lines, circles and squares: corners are told from curves."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import chains_model as CM
import refine_model as RM
import turns_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "cvsteer_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
F32 = np.float32
OFFSETS = dict(chain=0, flags=4, nb=8, nf=12, sin=16, cos=20, lb=24, lf=28)
SUMMARY_OFFSETS = dict(corners=0, eligible=4, sharpest=8, min_cos=12)
CFG = dict(radius=5, min_arm=5, nms=5, max_cos=M.COS45)


# ---- header, binding and build ----
def test_header_declares_the_call_and_the_records(tmp_path):
    text = open(os.path.join(ROOT, "include", "cvsteer_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int cvs_chain_turns\(cvs_handle h, const int32_t\* points, int n_points, const cvs_chain\* chains, int n_chains,\s*"
                     r"const float\* xy,\s*const cvs_turn_cfg\* cfg,\s*cvs_chain_turn\* table,\s*cvs_turn_summary\* summary,\s*int mem\);", plain)
    assert re.search(r"#define CVS_ABI_VERSION 2\b", text)
    src = os.path.join(str(tmp_path), "use.cpp")
    with open(src, "w") as f:
        f.write('#include <stddef.h>\n#include "cvsteer_hip.h"\n'
                'static_assert(sizeof(cvs_chain_turn) == 32 && sizeof(cvs_turn_summary) == 16 && sizeof(cvs_turn_cfg) == 16, "sizes");\n'
                'static_assert(CVS_TURN_CORNER == 1 && CVS_TURN_END == 2 && CVS_TURN_DEGENERATE == 4 && CVS_TURN_SHORT == 8 && '
                'CVS_TURN_NO_CHAIN == 16, "flags");\n'
                'static_assert(offsetof(cvs_turn_cfg, radius) == 0 && offsetof(cvs_turn_cfg, min_arm) == 4 && offsetof(cvs_turn_cfg, nms) == 8 && '
                'offsetof(cvs_turn_cfg, max_cos) == 12, "cfg");\n'
                + "".join('static_assert(offsetof(cvs_chain_turn, %s) == %d, "%s");\n' % (n, o, n) for n, o in OFFSETS.items())
                + "".join('static_assert(offsetof(cvs_turn_summary, %s) == %d, "%s");\n' % (n, o, n) for n, o in SUMMARY_OFFSETS.items()) +
                'int (*turns)(cvs_handle, const int32_t*, int, const cvs_chain*, int, const float*, const cvs_turn_cfg*, cvs_chain_turn*,'
                ' cvs_turn_summary*, int) = cvs_chain_turns;\n'
                'int main() { return turns == 0; }\n')
    subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), src], check=True)


def test_libraries_export_and_bind():
    import cvsteer_amd
    from cvsteer_amd import _lib as L
    assert L.SIGNATURES["cvs_chain_turns"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(L.TurnCfg),
                                                         C.c_void_p, C.c_void_p, C.c_int])
    assert C.sizeof(L.ChainTurn) == 32 == M.TURN_DTYPE.itemsize and C.sizeof(L.TurnSummary) == 16 == M.SUMMARY_DTYPE.itemsize
    assert C.sizeof(L.TurnCfg) == 16
    assert (L.TURN_CORNER, L.TURN_END, L.TURN_DEGENERATE, L.TURN_SHORT, L.TURN_NO_CHAIN) == (M.CORNER, M.END, M.DEGENERATE, M.SHORT, M.NO_CHAIN) \
        == (cvsteer_amd.TURN_CORNER, cvsteer_amd.TURN_END, cvsteer_amd.TURN_DEGENERATE, cvsteer_amd.TURN_SHORT, cvsteer_amd.TURN_NO_CHAIN)
    hip = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "cvsteer_amd", "libcvsteer_hip.so")], text=True)
    assert re.search(r" T cvs_chain_turns$", hip, re.M)
    so = os.path.join(ROOT, "cvsteer_amd", "libcvsteer.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cvsteer_amd", "facade"), "-s"])
    syms = subprocess.check_output(["nm", "-DC", "--defined-only", so], text=True)
    for cls in ("SteerableFiltersG2", "SteerableFiltersG4"):
        assert re.search(r" T fa::%s::cornerContours\(fa::Mat1f const&, std::vector<std::vector<fa::Point," % cls, syms), cls
    for cls in (cvsteer_amd.SteerableFiltersG2, cvsteer_amd.SteerableFiltersG4):
        assert all(callable(getattr(cls, name, None)) for name in ("chain_turns", "contour_corners"))
        assert cls.TURN_DTYPE == M.TURN_DTYPE and cls.TURN_SUMMARY_DTYPE == M.SUMMARY_DTYPE
        assert {n: cls.TURN_DTYPE.fields[n][1] for n in cls.TURN_DTYPE.names} == OFFSETS
        assert {n: cls.TURN_SUMMARY_DTYPE.fields[n][1] for n in cls.TURN_SUMMARY_DTYPE.names} == SUMMARY_OFFSETS
    assert [(n, getattr(L.ChainTurn, n).offset) for n, _ in L.ChainTurn._fields_] == list(OFFSETS.items())
    assert [(n, getattr(L.TurnSummary, n).offset) for n, _ in L.TurnSummary._fields_] == list(SUMMARY_OFFSETS.items())


def test_null_handle():
    from cvsteer_amd import _lib as L
    pts, tab = np.int32([[0, 0], [1, 0], [2, 0]]), np.int32([[0, 3, 0, 0]])
    rec = np.full((3, 8), -9, np.int32)
    cfg = L.TurnCfg(1, 1, 0, 0.5)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert L.lib().cvs_chain_turns(None, p(pts), 3, p(tab), 1, None, C.byref(cfg), p(rec), None, L.MEM_HOST) == L.E_BADARG
    assert (rec == -9).all()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_turn_kernels_use_no_scratch(tmp_path):
    path = os.path.join(str(tmp_path), "cvs_kernels_turns.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    "-I" + SRC, "-S", "--cuda-device-only", os.path.join(SRC, "cvs_kernels_turns.hip"), "-o", path], check=True,
                   stderr=subprocess.DEVNULL)
    text = open(path).read()
    scratch = {}
    for blk in text.split("  - .agpr_count:")[1:]:
        nm = re.search(r"\.name:\s+(\S+)", blk)
        ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        if nm and ps:
            scratch[nm.group(1)] = int(ps.group(1))
    for stem in ("k_turns", "k_turn_nms", "k_turn_summary"):
        assert any(stem in n for n in scratch), (stem, sorted(scratch))
    assert len(scratch) == 3 and all(v == 0 for v in scratch.values()), scratch


# ---- the model on its own: hand cases ----
def _one(points, closed=False, xy=None, **cfg):
    points = np.asarray(points, np.int32).reshape(-1, 2)
    return M.turns(points, np.int32([[0, len(points), M.CLOSED if closed else 0, 0]]), xy=xy, **cfg)


def test_model_a_right_angle_with_arms_of_three():
    """right along x, then down the screen: a clockwise turn, sin +1"""
    pts = [(0, 0), (1, 0), (2, 0), (3, 0), (3, 1), (3, 2), (3, 3)]
    t, s = _one(pts, radius=3, min_arm=3, nms=3, max_cos=0.5, summary=True)
    assert t["nb"].tolist() == [0, 1, 2, 3, 3, 3, 3] and t["nf"].tolist() == [3, 3, 3, 3, 2, 1, 0]
    v = t[3]
    assert (v["chain"], v["flags"], v["sin"], v["cos"], v["lb"], v["lf"]) == (0, M.CORNER, 1.0, 0.0, 2.0, 2.0)
    assert t["flags"].tolist() == [M.END | M.SHORT, M.SHORT, M.SHORT, M.CORNER, M.SHORT, M.SHORT, M.END | M.SHORT]
    assert np.isnan(t["sin"][[0, 6]]).all() and np.isnan(t["cos"][[0, 6]]).all()
    assert t["sin"].view(np.uint32)[0] == M.QNAN_BITS and (t["lb"][0], t["lf"][0], t["lb"][6], t["lf"][6]) == (0.0, 2.0, 2.0, 0.0)
    assert s.tolist() == [(1, 1, 3, 0.0)]
    back = _one(pts[::-1], radius=3, min_arm=3, nms=3, max_cos=0.5)[3]           # the other way round: counter-clockwise
    assert (back["sin"], back["cos"], back["flags"]) == (-1.0, 0.0, M.CORNER)
    assert _one(pts, radius=3, min_arm=3, nms=3, max_cos=-0.5)["flags"][3] == 0  # not sharp enough for this max_cos


def test_model_straight_reversed_and_degenerate():
    t = _one([(k, 2 * k) for k in range(7)], radius=2, min_arm=1, nms=0, max_cos=1.0)
    assert np.allclose(t["cos"][1:6], 1.0, atol=1e-7) and (t["sin"][1:6] == 0).all() and (t["flags"][1:6] == M.CORNER).all()   # nms 0: all of them
    t = _one([(0, 0), (1, 0), (2, 0), (1, 0), (0, 0)], radius=2, min_arm=2, nms=2, max_cos=0.0)
    assert (t["cos"][2], t["flags"][2]) == (-1.0, M.CORNER)                      # there and back again
    # an arm whose centroid is the point itself: DEGENERATE, not a corner, NaN
    t = _one([(0, 0), (1, 0), (0, 0), (5, 5), (6, 5)], radius=2, min_arm=1, nms=0, max_cos=1.0)
    assert t["flags"][2] & M.DEGENERATE == 0 and t["nb"][2] == 2
    t = _one([(1, 0), (-1, 0), (0, 0), (5, 5), (6, 5)], radius=2, min_arm=1, nms=0, max_cos=1.0)
    assert t["flags"][2] == M.DEGENERATE and np.isnan(t["cos"][2]) and (t["lb"][2], t["nb"][2]) == (0.0, 2)
    xy = F32([[0, 0], [1, 0], [np.nan, 0], [3, 0], [4, 0], [5, 0]])
    t = _one([(k, 0) for k in range(6)], xy=xy, radius=1, min_arm=1, nms=0, max_cos=1.0)
    assert t["flags"].tolist() == [M.END | M.SHORT, M.DEGENERATE, M.DEGENERATE, M.DEGENERATE, M.CORNER, M.END | M.SHORT]


def test_model_closed_chains_and_short_chains():
    ring = [(0, 0), (1, 0), (2, 0), (2, 1), (2, 2), (1, 2), (0, 2), (0, 1)]
    t, s = _one(ring, closed=True, radius=5, min_arm=1, nms=5, max_cos=0.5, summary=True)
    assert (t["nb"] == 3).all() and (t["nf"] == 3).all()                         # (L - 1) / 2: the arms never share a point
    assert (t["flags"] & M.INELIGIBLE == 0).all() and (t["sin"] > 0).all()      # clockwise on the screen all the way round
    assert s["eligible"][0] == 8 and s["sharpest"][0] == int(np.argmin(t["cos"]))
    E = M.END | M.SHORT                                                          # a missing arm is a short arm
    for n, closed, want in ((1, False, [E]), (2, False, [E] * 2), (1, True, [E]), (2, True, [E] * 2), (3, True, [0] * 3)):
        t = _one([(k, k * k) for k in range(n)], closed=closed, radius=5, min_arm=1, nms=0, max_cos=-1.0)
        assert t["flags"].tolist() == want, (n, closed)
    t = _one([(k, 0) for k in range(12)], radius=5, min_arm=3, nms=0, max_cos=1.0)
    assert [bool(f & M.SHORT) for f in t["flags"]] == [True] * 3 + [False] * 6 + [True] * 3


def test_model_plateau_keeps_the_first():
    """two equal cosines side by side: the strict comparison backwards keeps the first only"""
    pts = [(0, 0), (1, 0), (2, 0), (3, 1), (4, 1), (5, 1)]                        # symmetric under a half turn: cos[2] == cos[3]
    t = _one(pts, radius=2, min_arm=2, nms=2, max_cos=1.0)
    assert t["cos"][2] == t["cos"][3] and t["cos"][2] < 1 and (t["flags"][2], t["flags"][3]) == (M.CORNER, 0)
    assert (_one(pts, radius=2, min_arm=2, nms=0, max_cos=1.0)["flags"][2:4] == M.CORNER).all()


def test_model_tables_a_device_call_accepts():
    pts = np.int32([(k, 0) for k in range(10)])
    tab = np.int32([[0, 4, 0, 0], [4, 3, 0, 0], [8, 5, 0, 0]])                  # a gap at 7, and the last entry leaves the array
    t, s = M.turns(pts, tab, radius=1, min_arm=1, nms=0, max_cos=1.0, summary=True)
    assert t["chain"].tolist() == [0] * 4 + [1] * 3 + [-1] * 3
    gone = t[7:]
    assert (gone["flags"] == M.NO_CHAIN).all() and not gone["nb"].any() and not gone["lb"].any() and np.isnan(gone["cos"]).all()
    assert s.tolist()[2] == (0, 0, -1, np.inf) and s["eligible"].tolist() == [2, 1, 0]
    assert M.find_chain([0, 4, 8], np.arange(-1, 10)).tolist() == [0] + [0] * 4 + [1] * 4 + [2] * 2


# ---- geometry on hand-made ordered lists ----
def _segment(x0, y0, x1, y1, n):
    pts = [(round(x0 + (x1 - x0) * i / n), round(y0 + (y1 - y0) * i / n)) for i in range(n + 1)]
    return [p for k, p in enumerate(pts) if k == 0 or p != pts[k - 1]]


def _line(deg, length=60):
    a = np.deg2rad(deg)
    return _segment(100.0, 100.0, 100.0 + length * np.cos(a), 100.0 + length * np.sin(a), length)


def _circle(radius):
    """the digital circle round (100, 100) as an 8-connected cycle without staircase corners: one octant by stepping its major axis,
    x = round(sqrt(R^2 - y^2)) while y <= x, the other seven by symmetry"""
    octant = []
    for y in range(radius + 1):
        x = round(np.sqrt(radius * radius - y * y))
        if y > x:
            break
        octant.append((x, y))
    quadrant = octant + [(y, x) for x, y in reversed(octant)]
    pts = []
    for turn in range(4):
        for x, y in quadrant:
            for _ in range(turn):
                x, y = -y, x
            if not pts or pts[-1] != (100 + x, 100 + y):
                pts.append((100 + x, 100 + y))
    return pts[:-1] if pts[-1] == pts[0] else pts


def _square(deg, side=40, centre=(50.0, 50.0)):
    a = np.deg2rad(deg)
    h = side / 2.0
    vertices = [(centre[0] + x * np.cos(a) - y * np.sin(a), centre[1] + x * np.sin(a) + y * np.cos(a)) for x, y in ((-h, -h), (h, -h), (h, h), (-h, h))]
    pts = []
    for k in range(4):
        (x0, y0), (x1, y1) = vertices[k], vertices[(k + 1) % 4]
        pts += [p for p in _segment(x0, y0, x1, y1, side) if not pts or p != pts[-1]]
    return (pts[:-1] if pts[-1] == pts[0] else pts), vertices


def _angle(rec):
    return float(np.rad2deg(np.arctan2(rec["sin"], rec["cos"])))


def test_geometry_lines_circles_squares():
    """radius = min_arm = nms = 5, max_cos = cos 45 deg, on integer points.  What is asserted: no corner on a digital line at 0, 3, ..., 177
    degrees, none on a digital circle of radius 8, 16, 32, and exactly one within 2 px of each vertex of a square of side 40 at 0, 5, ...,
    85 degrees, no other.  The figures, as this model measures them (printed by the test):
        lines:    the smallest interior (eligible) cos is 0.89443 (26.57 deg)
        circles:  the smallest cos is 0.76528, 0.88099 and 0.92848 for radius 8, 16 and 32 (44, 92 and 180 points)
        squares:  the corner lies at most 1.04 px from its vertex (0 px at 0 degrees), its turn is 75.79 .. 102.53 deg (90.00 at 0 degrees)
    (The prototype behind the feature request quoted 0.94868 for the lines, 0.7399, 0.7399, 0.7653 for the circles and distance 0, turn 90
    for the squares, from lists of its own making; the conditions hold on both, the figures above are those of the lists made here.)"""
    worst = 1.0
    for deg in range(0, 180, 3):
        t = _one(_line(deg), **CFG)
        el = t[(t["flags"] & M.INELIGIBLE) == 0]
        assert len(el) == len(t) - 10 >= 30 and not (t["flags"] & M.CORNER).any(), deg
        worst = min(worst, float(el["cos"].min()))
    print("lines: smallest eligible cos %.5f (%.2f deg)" % (worst, np.rad2deg(np.arccos(worst))))
    for radius in (8, 16, 32):
        t = _one(_circle(radius), closed=True, **CFG)
        assert (t["flags"] & M.INELIGIBLE == 0).all() and not (t["flags"] & M.CORNER).any(), radius
        print("circle of radius %d: %d points, smallest cos %.5f" % (radius, len(t), float(t["cos"].min())))
    far, lo, hi = 0.0, 180.0, 0.0
    for deg in range(0, 90, 5):
        pts, vertices = _square(deg)
        t = _one(pts, closed=True, **CFG)
        at = np.nonzero(t["flags"] & M.CORNER)[0]
        assert len(at) == 4, (deg, at)
        dist = np.array([[np.hypot(pts[i][0] - vx, pts[i][1] - vy) for vx, vy in vertices] for i in at])
        assert sorted(dist.argmin(axis=1).tolist()) == [0, 1, 2, 3] and (dist.min(axis=1) <= 2.0).all(), (deg, dist.min(axis=1))
        far = max(far, float(dist.min(axis=1).max()))
        lo, hi = min([lo] + [_angle(t[i]) for i in at]), max([hi] + [_angle(t[i]) for i in at])
        if deg == 0:
            assert dist.min(axis=1).max() == 0.0 and [_angle(t[i]) for i in at] == [90.0] * 4
    print("squares: corner at most %.2f px from its vertex, turn %.2f .. %.2f deg" % (far, lo, hi))


# ---- recorded, not asserted: ridges with a corner through the CPU models ----
@pytest.mark.parametrize("name, deg_in, deg_out", [("L-shaped", 0.0, 90.0), ("60 degree", 0.0, 60.0), ("120 degree", 0.0, 120.0)])
def test_ridge_corners_recorded(name, deg_in, deg_out):
    """Ridges that turn by 90 degrees (an L), by 60 and by 120 degrees on 48 x 48, through contour_model, chains_model and refine_model, then
    the turns model on the integer and on the sub-pixel points.  RECORDED, not asserted: the figures are printed, and quoted in DESIGN.md
    section 6 as model figures on synthetic ridges.  As this model measures them (corner's distance from the true vertex, its turn):
        L-shaped    integer 0.316 px, 90.00 deg     sub-pixel 0.445 px, 77.96 deg
        60 degree   integer 0.316 px, 56.31 deg     sub-pixel 0.314 px, 51.64 deg
    (near the vertex the analytic theta of the nearer ray flips from one arm's normal to the other's, so the sub-pixel offsets there point
    across the wrong arm: the refinement gains nothing AT a corner, the integer points are as good)
        120 degree  no corner on either: the thinned ridge has a spur at so sharp a vertex, the chains are cut at that junction, and a
                    chain's ends have no turn -- a caller joins chains at junctions before it asks for corners there"""
    img, theta, (vx, vy), mask = M.ridge_case(deg_in, deg_out)
    pts, chains = CM.chains(mask)
    xy, _ = RM.refine(pts, img, theta)
    for what, sub in (("integer points", None), ("sub-pixel points", xy)):
        t = M.turns(pts, chains, xy=sub, **CFG)
        at = np.nonzero(t["flags"] & M.CORNER)[0]
        if len(at) == 0:
            print("%s ridge, %s: %d chains %s, no corner" % (name, what, len(chains), chains[:, 1].tolist()))
            continue
        pos = pts.astype(np.float64) if sub is None else sub.astype(np.float64)
        best = at[np.argmin(t["cos"][at])]
        print("%s ridge, %s: %d chain(s), %d corner(s), the sharpest %.3f px from the true vertex, turn %.2f deg (true %.0f)"
              % (name, what, len(chains), len(at), float(np.hypot(pos[best, 0] - vx, pos[best, 1] - vy)), _angle(t[best]), deg_out - deg_in))
