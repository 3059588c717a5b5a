"""GPU tests (-m gpu): the HIP kernels and the C++ facade held to planes that the REFERENCE'S OWN source files wrote
(tests/golden/ref_run/; see tests/test_reference_run_cpu.py and oracle/ref_run.mk for how they were made).  Only the committed fixtures
are read here.  Each test is a handful of launches on 24 x 70 planes: 24 rows put G4 on its strip path, 70 columns cross the 64-column
wave seam, set_strip_rows(10) cuts three strips, the bottom rows are an exact zero band.

What this pins that the oracle comparisons cannot: the oracle and the kernels were written from the same reading of the reference, so a
slip in the reading (a tap pairing, a steering sign -- the global sign of the H bank, G4's pairing) is in both; the fixture is not.

Bounds.  Basis planes: 1e-5 * max(1, max|plane|) (the north-star bound of test_basis_on_fish_relative_tolerance).  g, h steered from the
image: 1e-5 * max(1, max|g|, max|h|).  Entries that take planes, fed the fixture's own inputs: those of test_mag_phase_weights_find
(magnitude np.allclose(atol=1e-6), phase bit for bit, weights and unit-energy maps 1e-6, maps 1e-6 * max(1, max e)); wrap bit for
bit.  Products of planes from the image: the first-order propagation written out in test_gpu_bench_instances.py, with d_b = this
launch's measured basis distance + 2e-7 * max(1, bmax) (see _Prop), on every pixel with strength > 1e-3 * bmax^2 and magnitude >
1e-3 * bmax; angles modulo their cut.

On the crafted phase plane the float neighbours of +-float(pi / 2) decide the gate of phaseWeights(0, signed): |p| = float(pi / 2)
= 0x3fc90fdb is NOT above the gate and keeps cos^2 = 1.9e-15 (nonzero bits), the next float up, 0x3fc90fdc, is and gives +0, the next
float down, 0x3fc90fda, gives cos^2 of its own.  For (pi / 2, unsigned) the same happens at p = +-0 and +-float(pi), for (pi, signed) at
float(pi / 2).  Each side is asserted bit for bit against what the reference's run left there.

Largest observed fraction of each bound (MI355X; this module prints them):
  basis G2, every launch and input form   0.020 (the same in all 25 forms)   basis G4   0.031   generic widths   0.023 (G2) / 0.026 (G4)
  steer from the image (g, h)             G2 0.025, G4 0.031 (steer, steer_bank, setup_steer, host and device alike)
  steer(Point)                            g, h 0.010   e 0.006   magnitude 0.041   phase 0.020
  entries that take planes                phaseWeights 0.119   find on unit energy 0.358   find on the image's magnitude 0.306
                                          magnitude np.allclose, phase / wrap / every gate side bit for bit
  products of planes                      C1 / C2 / C3 0.033 / 0.037 / 0.017   strength 0.035   theta 0.026
                                          g, h 0.126   e 0.022   magnitude 0.118   phase 0.217   the three maps 0.003
  facade through ref_sequence             the same figures as the Python calls: 0.358 (find on unit energy), 0.217 (phase)"""
import os
import subprocess

import numpy as np
import pytest
import torch

import cvsteer_amd as cv
import orientation_model as O
import ref_run_fixture as R
from cvsteer_amd import _lib as L
from helpers import angle_diff

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
TOL = 1e-5
WORST = {}


@pytest.fixture(scope="module")
def run(golden_dir):
    planes, points = R.load(golden_dir)
    for p in planes.values():
        p.setflags(write=False)
    return planes, points


def _np(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)      # a writable copy: the fixtures are read-only


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _stack(planes, stem, n):
    return np.stack([planes["%s_%d" % (stem, i)] for i in range(n)])


def _note(stage, what, frac):
    """remember and print the largest fraction of its bound a stage has used; a NaN (a lost pixel) is a miss"""
    frac = float(frac)
    assert not np.isnan(frac), (stage, what)
    WORST[stage] = max(WORST.get(stage, 0.0), frac)
    print("kernel vs reference run, %-14s %-52s %.3g of the bound" % (stage, what, frac))
    return frac


def _hold(stage, what, got, want, bound):
    """max |got - want| / bound over all pixels (bound: a number or a plane); -> the largest |got - want|"""
    got, want = _np(got).astype(F64), np.asarray(want, F64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    d = np.abs(got - want)
    assert _note(stage, what, (d / bound).max()) <= 1.0, (stage, what)
    return float(d.max())


def _hold_basis(stage, what, f, want):
    """the handle's basis planes against the fixture's, plane by plane at 1e-5 * max(1, max|plane|) -> the largest distance (d_b)"""
    worst = 0.0
    for p in range(len(want)):
        worst = max(worst, _hold(stage, "%s, plane %d" % (what, p), f.basis(p), want[p], TOL * max(1.0, float(np.abs(want[p]).max()))))
    return worst


def _roi(a, device):
    """the same pixels as a pitched view inside a larger plane (a cv::Mat ROI: step > cols * 4)"""
    big = np.full((a.shape[0] + 5, a.shape[1] + 11), 7, a.dtype)
    big[2:2 + a.shape[0], 6:6 + a.shape[1]] = a
    if device:
        return _dev(big)[2:2 + a.shape[0], 6:6 + a.shape[1]]
    return big[2:2 + a.shape[0], 6:6 + a.shape[1]]


# ----------------------------------------------------------------------------- basis
def test_g2_basis_in_every_launch_and_input_form(run):
    planes, _ = run
    img, want = planes["image"], _stack(planes, "g2_basis", 7)
    forms = [("default handle", {}, None)]
    forms += [("strip rows %d" % sr, {}, sr) for sr in (1, 10, 1000)]
    forms += [("state layout %d" % k, {L.OPT_STATE_LAYOUT: k}, None) for k in range(4)]
    inputs = (("host plane", np.array(img)), ("device plane", _dev(img)), ("host ROI", _roi(img, False)), ("device ROI", _roi(img, True)),
              ("byte image widened, host", img.astype(np.uint8)), ("byte image widened, device", _dev(img.astype(np.uint8))))
    for what, opts, sr in forms:
        for iname, src in inputs if not opts and sr is None else inputs[:2]:
            f = cv.SteerableFiltersG2(None, *R.G2_DEFAULT)
            for o, v in opts.items():
                f.set_option(o, v)
            if sr is not None:
                f.set_strip_rows(sr)
            f.setup(src)
            _hold_basis("basis G2", "%s, %s" % (what, iname), f, want)
    # every layout and strip height gives the same planes as the default handle, bit for bit
    f0 = cv.SteerableFiltersG2(img, *R.G2_DEFAULT)
    ref = np.stack([f0.basis(p) for p in range(7)])
    f1 = cv.SteerableFiltersG2(None, *R.G2_DEFAULT)
    f1.set_strip_rows(10)
    f1.setup(img)
    assert np.array_equal(_bits(np.stack([f1.basis(p) for p in range(7)])), _bits(ref))


def test_g4_basis_pair_launch_and_setup_steer(run):
    planes, _ = run
    img, want = planes["image"], _stack(planes, "g4_basis", 11)
    for iname, src in (("host plane", np.array(img)), ("device plane", _dev(img)), ("device ROI", _roi(img, True))):
        f = cv.SteerableFiltersG4(src, *R.G4_DEFAULT)
        _hold_basis("basis G4", "setup, " + iname, f, want)
        for sr in (1, 10):
            f = cv.SteerableFiltersG4(None, *R.G4_DEFAULT)
            f.set_strip_rows(sr)
            f.setup(src)
            _hold_basis("basis G4", "setup, strip rows %d, %s" % (sr, iname), f, want)
        f = cv.SteerableFiltersG4(None, *R.G4_DEFAULT)
        g, h = f.setup_steer(src, 0.3)
        _hold_basis("basis G4", "setup_steer, " + iname, f, want)
        scale = TOL * max(1.0, float(np.abs(planes["g4_s0_g"]).max()), float(np.abs(planes["g4_s0_h"]).max()))
        _hold("steer", "G4 setup_steer(0.3) g, " + iname, g, planes["g4_s0_g"], scale)
        _hold("steer", "G4 setup_steer(0.3) h, " + iname, h, planes["g4_s0_h"], scale)


def test_generic_width_basis_and_steer(run):
    planes, _ = run
    img = planes["image"]
    for cls, cfg, stem, n in ((cv.SteerableFiltersG2, R.G2_GENERIC, "g2w3", 7), (cv.SteerableFiltersG4, R.G4_GENERIC, "g4w4", 11)):
        for iname, src in (("host plane", np.array(img)), ("device plane", _dev(img))):
            f = cls(src, *cfg)
            _hold_basis("basis generic", "%s (%d, %.2f), %s" % (stem, cfg[0], cfg[1], iname), f, _stack(planes, stem + "_basis", n))
            g, h = f.steer(0.3)
            wg, wh = planes[stem + "_g"], planes[stem + "_h"]
            scale = TOL * max(1.0, float(np.abs(wg).max()), float(np.abs(wh).max()))
            _hold("steer", "%s steer(0.3) g, %s" % (stem, iname), g, wg, scale)
            _hold("steer", "%s steer(0.3) h, %s" % (stem, iname), h, wh, scale)


# ----------------------------------------------------------------------------- steer from the image
def _gh_scale(wg, wh):
    return TOL * max(1.0, float(np.abs(wg).max()), float(np.abs(wh).max()))


def test_g2_steer_from_the_image(run):
    """the relative signs of the H bank (and of g against h) as the reference's run has them: steer(theta), steer(map), the fused
    setup_steer and the steering bank"""
    planes, _ = run
    img = planes["image"]
    for iname, src, tmap in (("host", np.array(img), np.array(planes["theta_map"])), ("device", _dev(img), _dev(planes["theta_map"]))):
        f = cv.SteerableFiltersG2(src, *R.G2_DEFAULT)
        bank = f.steer_bank(np.array(R.THETAS, F32))
        for k, theta in enumerate(R.THETAS):
            wg, wh = planes["g2_s%d_g" % k], planes["g2_s%d_h" % k]
            assert np.array_equal(_bits(wg), _bits(planes["g2_s%d_g5" % k])) and np.array_equal(_bits(wh), _bits(planes["g2_s%d_h5" % k]))
            s = _gh_scale(wg, wh)
            g, h = f.steer(float(theta))
            _hold("steer", "G2 steer(%.2f) g, %s" % (theta, iname), g, wg, s)
            _hold("steer", "G2 steer(%.2f) h, %s" % (theta, iname), h, wh, s)
            _hold("steer", "G2 steer_bank[%d] g, %s" % (k, iname), bank[0][k], wg, s)
            _hold("steer", "G2 steer_bank[%d] h, %s" % (k, iname), bank[1][k], wh, s)
            f2 = cv.SteerableFiltersG2(None, *R.G2_DEFAULT)
            g, h = f2.setup_steer(src, float(theta), flags=cv.SETUP_FULL)
            _hold("steer", "G2 setup_steer(%.2f) g, %s" % (theta, iname), g, wg, s)
            _hold("steer", "G2 setup_steer(%.2f) h, %s" % (theta, iname), h, wh, s)
        wg, wh = planes["g2_map_g"], planes["g2_map_h"]
        g, h = f.steer(tmap)
        _hold("steer", "G2 steer(map) g, " + iname, g, wg, _gh_scale(wg, wh))
        _hold("steer", "G2 steer(map) h, " + iname, h, wh, _gh_scale(wg, wh))


def test_g4_steer_from_the_image(run):
    """G4's pairing of tap vectors with planes and of planes with steering weights, as the reference's run has them"""
    planes, _ = run
    img = planes["image"]
    for iname, src, tmap in (("host", np.array(img), np.array(planes["theta_map"])), ("device", _dev(img), _dev(planes["theta_map"]))):
        f = cv.SteerableFiltersG4(src, *R.G4_DEFAULT)
        bank = f.steer_bank(np.array([0.3, -2.0], F32))
        for k, (theta, stem) in enumerate(((0.3, "g4_s0"), (-2.0, "g4_s1"))):
            wg, wh = planes[stem + "_g"], planes[stem + "_h"]
            g, h = f.steer(theta)
            _hold("steer", "G4 steer(%.1f) g, %s" % (theta, iname), g, wg, _gh_scale(wg, wh))
            _hold("steer", "G4 steer(%.1f) h, %s" % (theta, iname), h, wh, _gh_scale(wg, wh))
            _hold("steer", "G4 steer_bank[%d] g, %s" % (k, iname), bank[0][k], wg, _gh_scale(wg, wh))
            _hold("steer", "G4 steer_bank[%d] h, %s" % (k, iname), bank[1][k], wh, _gh_scale(wg, wh))
        wg, wh = planes["g4_map_g"], planes["g4_map_h"]
        g, h = f.steer(tmap)
        _hold("steer", "G4 steer(map) g, " + iname, g, wg, _gh_scale(wg, wh))
        _hold("steer", "G4 steer(map) h, " + iname, h, wh, _gh_scale(wg, wh))


def test_g2_steer_point(run):
    planes, points = run
    f = cv.SteerableFiltersG2(np.array(planes["image"]), *R.G2_DEFAULT)
    want_b = _stack(planes, "g2_basis", 7)
    bmax = float(np.abs(want_b).max())
    d_b = _hold_basis("basis G2", "setup for steer(Point)", f, want_b) + 2e-7 * max(1.0, bmax)      # as in _Prop
    for k, theta in enumerate(R.THETAS):
        s = _gh_scale(planes["g2_s%d_g" % k], planes["g2_s%d_h" % k])
        for i, (x, y) in enumerate(R.POINTS):
            want = points[k, i]
            g2, h2 = f.steer_point((x, y), float(theta))
            g, h, e, m, p = f.steer_point((x, y), float(theta), full=True)
            assert (g2, h2) == (g, h)
            tag = "(%d, %d) at %.2f" % (x, y, theta)
            _hold("steer(Point)", tag + " g", F32(g), want[2], s)
            _hold("steer(Point)", tag + " h", F32(h), want[3], s)
            # first order, as in _Prop: |de| <= 3 |dC|, |dC| <= 11.5 bmax d_b; |dm| <= sqrt(2) * 4 d_b; m |dphase| <= sqrt(2) * 4 d_b
            _hold("steer(Point)", tag + " e", F32(e), want[4], 3 * 11.5 * bmax * d_b)
            _hold("steer(Point)", tag + " magnitude", F32(m), want[5], np.sqrt(2) * 4 * d_b)
            if want[5] > 1e-3 * bmax:
                dp = float(angle_diff(np.array([p], F32), want[6:7], 2 * np.pi)[0])
                assert _note("steer(Point)", tag + " phase", dp / (np.sqrt(2) * 4 * d_b / float(want[5]))) <= 1.0
            if y >= R.ROWS - R.ZERO_ROWS + 4:
                assert g == 0 and h == 0 and e == 0 and m == 0      # the zero band


# ----------------------------------------------------------------------------- entries that take planes
@pytest.mark.parametrize("device", [False, True])
def test_entries_that_take_planes(run, device):
    planes, _ = run
    put = _dev if device else np.array
    f = cv.SteerableFiltersG2(None)
    g, h = planes["craft_g"], planes["craft_h"]
    m, p = (_np(x) for x in f.computeMagnitudeAndPhase(put(g), put(h)))
    assert np.allclose(m, planes["craft_mag"], atol=1e-6, equal_nan=True)
    fin = np.isfinite(m)
    _note("planes", "magnitude, crafted (g, h)", (np.abs(m[fin] - planes["craft_mag"][fin]) / (1e-6 + 1e-5 * np.abs(planes["craft_mag"][fin]))).max())
    assert np.array_equal(_bits(p), _bits(planes["craft_phase_out"]))            # same polynomial, same op order: bit for bit
    nan = np.isnan(g)
    assert nan.sum() == 1 and (_bits(p)[nan] == 0).all() and np.isfinite(p).all()     # patchNaNs
    assert np.array_equal(_bits(_np(f.wrap(put(planes["craft_angle"])))), _bits(planes["craft_wrap"]))
    ph = planes["craft_phase"]
    sp = R.phase_specials()
    near_gate = np.zeros(ph.shape, bool)
    near_gate.flat[:sp.size] = True                                              # 0, +-pi/2, +-pi and their float neighbours
    for k, (phi, signum) in enumerate(R.PHASE_WEIGHTS):
        lam, want = _np(f.phaseWeights(put(ph), float(phi), signum)), planes["craft_pw%d" % k]
        _hold("planes", "phaseWeights(%.2f, %s), away from the gate" % (phi, signum), np.where(near_gate, 0, lam), np.where(near_gate, 0, want), 1e-6)
        _hold("planes", "phaseWeights(%.2f, %s), at the specials" % (phi, signum), lam[near_gate], want[near_gate], 1e-6)
        # the gate's side, bit for bit: which pixels are an exact +0 (gated, or cos^2 underflowed nowhere here) and which are not
        assert np.array_equal(_bits(lam)[near_gate] == 0, _bits(want)[near_gate] == 0), (phi, signum)
    lam = _np(f.phaseWeights(put(ph), 0.0, True))
    hp = R.HALF_PI32
    for v, gated in ((hp, False), (-hp, False), (np.nextafter(hp, F32(2)), True), (np.nextafter(-hp, F32(-2)), True),
                     (np.nextafter(hp, F32(0)), False), (np.nextafter(-hp, F32(0)), False)):
        at = ph == v
        assert at.any() and ((_bits(lam)[at] == 0).all() if gated else (_bits(lam)[at] != 0).all()), (float(v), gated)
        assert np.array_equal(_bits(lam)[at], _bits(planes["craft_pw1"])[at]), float(v)
    ones = np.ones_like(ph)
    names = ("craft_edges", "craft_dark", "craft_bright")
    outs = [_np(o) for o in f.find(put(ones), put(ph))]
    for got, n in zip(outs, names):
        _hold("planes", "find on unit energy, " + n, got, planes[n], 1e-6)
    assert np.array_equal(_np(f.findEdges(put(ones), put(ph))), outs[0])
    assert np.array_equal(_np(f.findDarkLines(put(ones), put(ph))), outs[1])
    assert np.array_equal(_np(f.findBrightLines(put(ones), put(ph))), outs[2])
    e, p2 = planes["g2_dom_mag"], planes["g2_dom_phase"]
    for got, n in zip(f.find(put(e), put(p2)), ("g2_find_edges", "g2_find_dark", "g2_find_bright")):
        _hold("planes", "find on the image's magnitude, " + n, got, planes[n], 1e-6 * max(1.0, float(e.max())))
    for stem in ("g2_s0", "g2_map"):
        m, p = (_np(x) for x in f.computeMagnitudeAndPhase(put(planes[stem + "_g5"]), put(planes[stem + "_h5"])))
        assert np.allclose(m, planes[stem + "_mag"], atol=1e-6) and np.array_equal(_bits(p), _bits(planes[stem + "_phase"])), stem


# ----------------------------------------------------------------------------- products of planes, from the image
class _Prop:
    """The first-order propagation of test_gpu_bench_instances.py (test_state_kept_batch ..., the comment above `bound = 2.5 * d_b ...`),
    per pixel, for a launch whose basis planes lie within d_b of the fixture's:
      |dC1|, |dC2|, |dC3| <= 5.75 * 2 * bmax * d_b = dC      (coefficient sums 4, 2.875, 5.75; products of two planes)
      |d strength|        <= sqrt(2) dC                      (a hypot of C2, C3)
      |d theta|           <= 0.5 sqrt(2) dC / strength
      e at a given angle  <= 3 dC                            (C1 + cos C2 + sin C3)
      e at theta          <= 3 dC + 2 (|C2| + |C3|) |d theta| <= 3 dC + 2 sqrt(2) strength |d theta| = 5 dC
      g, h at a given angle <= 4 d_b                         (sum of |weights| <= 4)
      g, h at theta       <= 4 d_b + 12 bmax |d theta| = dG
      magnitude           <= sqrt(2) |dg|;  magnitude * |d phase| <= sqrt(2) |dg|
      maps                <= sqrt(2) |dg| + magnitude |d phase| <= 2.5 * d_b * (4 + 98 bmax^2 / strength)   (the existing bound)
    d_b = the basis distance measured in this test for this launch + 2e-7 * max(1, bmax): one float32 ulp of the epilogue's own
    arithmetic (and of the run's: its eager sums and a folded sum differ by an ulp).  Held on every pixel with strength >
    1e-3 * bmax^2 and magnitude > 1e-3 * bmax."""

    def __init__(self, planes, measured):
        b = _stack(planes, "g2_basis", 7)
        self.bmax = float(np.abs(b).max())
        self.d_b = measured + 2e-7 * max(1.0, self.bmax)
        self.st = planes["g2_strength"].astype(F64)
        self.dC = 5.75 * 2 * self.bmax * self.d_b
        self.strong = self.st > 1e-3 * self.bmax ** 2
        with np.errstate(divide="ignore"):
            self.dtheta = 0.5 * np.sqrt(2) * self.dC / self.st
        self.dG = 4 * self.d_b + 12 * self.bmax * self.dtheta
        self.maps = 2.5 * self.d_b * (4.0 + 98.0 * self.bmax ** 2 / np.maximum(self.st, 1e-3 * self.bmax ** 2))
        self.zero = slice(R.ROWS - R.ZERO_ROWS + 4, R.ROWS)

    def hold(self, what, got, want, bound, where=None):
        got, want = _np(got).astype(F64), np.asarray(want, F64)
        where = np.ones(want.shape, bool) if where is None else where
        r = np.abs(got - want) / bound
        assert _note("products", what, r[where].max()) <= 1.0, what

    def hold_angle(self, what, got, want, period, bound, where):
        got = _np(got)
        d = O.theta_error(got, want) if period == np.pi else angle_diff(got, np.asarray(want), period)
        assert _note("products", what, (d / bound)[where].max()) <= 1.0, what

    def orientation(self, what, f, planes):
        for k, c in enumerate(f.coefficients()):
            self.hold("%s C%d" % (what, k + 1), c, planes["g2_c%d" % (k + 1)], self.dC)
        st, th = _np(f.getDominantOrientationStrength()), _np(f.getDominantOrientationAngle())
        self.hold(what + " strength", st, planes["g2_strength"], np.sqrt(2) * self.dC)
        self.hold_angle(what + " theta", th, planes["g2_theta"], np.pi, self.dtheta, self.strong)
        # the zero band: +0 strength and theta 0 exactly, as the run has them
        assert (_bits(planes["g2_strength"])[self.zero] == 0).all() and (_bits(planes["g2_theta"])[self.zero] == 0).all()
        assert (_bits(st)[self.zero] == 0).all() and (th[self.zero] == 0).all() and not np.signbit(th[self.zero]).any(), what

    def five(self, what, outs, planes, stem, at_theta):
        """g, h, e, magnitude, phase of a steer: at a given angle, or at the launch's own dominant angle (at_theta)"""
        g, h, e, m, p = (_np(o) for o in outs)
        wm = planes[stem + "_mag"].astype(F64)
        dg = self.dG if at_theta else 4 * self.d_b
        where = (self.strong if at_theta else np.ones(wm.shape, bool))
        # within reach of the cut theta = +-pi/2 the two sides differ by the sign of h, and so of the phase, alone (g is even under
        # theta -> theta + pi, h odd): |h| and |phase| are compared on those pixels, h and the phase themselves everywhere else
        cut = at_theta & (np.abs(planes["g2_theta"].astype(F64)) > np.pi / 2 - 2 * self.dtheta - 1e-6)
        fold = lambda a: np.where(cut, np.abs(a), a)
        self.hold(what + " g", g, planes[stem + "_g5"], dg, where)
        self.hold(what + " h", fold(h), fold(planes[stem + "_h5"]), dg, where)
        self.hold(what + " e", e, planes[stem + "_e"], 5 * self.dC if at_theta else 3 * self.dC, where)
        self.hold(what + " magnitude", m, wm, np.sqrt(2) * dg, where)
        ok = where & (wm > 1e-3 * self.bmax)
        with np.errstate(divide="ignore", invalid="ignore"):
            bound = np.sqrt(2) * dg / wm
        want_p = planes[stem + "_phase"]
        self.hold_angle(what + " phase", fold(p), fold(want_p), 2 * np.pi, bound, ok)
        return ok

    def three(self, what, outs, planes, ok):
        for got, n in zip(outs, ("g2_find_edges", "g2_find_dark", "g2_find_bright")):
            self.hold("%s %s" % (what, n[8:]), got, planes[n], self.maps, ok)


def test_products_of_planes_from_the_image(run):
    planes, _ = run
    img, want_b = planes["image"], _stack(planes, "g2_basis", 7)
    for iname, src in (("host", np.array(img)), ("device", _dev(img))):
        f = cv.SteerableFiltersG2(src, *R.G2_DEFAULT)
        pr = _Prop(planes, _hold_basis("basis G2", "setup(FULL) for the products, " + iname, f, want_b))
        pr.orientation("setup, " + iname, f, planes)
        for k, theta in enumerate(R.THETAS):
            pr.five("steer(%.2f, full), %s" % (theta, iname), f.steer(float(theta), full=True), planes, "g2_s%d" % k, False)
        tmap = planes["theta_map"]
        pr.five("steer(map, full), " + iname, f.steer(_dev(tmap) if iname == "device" else np.array(tmap), full=True), planes, "g2_map", False)
        outs = f.steer(None, full=True)                                   # at its own dominant angle
        ok = pr.five("steer(own theta, full), " + iname, outs, planes, "g2_dom", True)
        pr.three("find(own magnitude, phase), " + iname, f.find(outs[3], outs[4]), planes, ok)
        for persist in (True, False):                                     # pipeline(): fused with the state kept, and outputs only
            f = cv.SteerableFiltersG2(None, *R.G2_DEFAULT)
            f.set_persist(persist)
            outs = f.pipeline(src)
            what = "pipeline(%s), %s" % ("state kept" if persist else "outputs only", iname)
            measured = _hold_basis("basis G2", what, f, want_b) if persist else pr.d_b - 2e-7 * max(1.0, pr.bmax)
            pp = _Prop(planes, measured)
            if persist:
                pp.orientation(what, f, planes)
            ok = pp.five(what, outs[:5], planes, "g2_dom", True)
            pp.three(what, outs[5:], planes, ok)


# ----------------------------------------------------------------------------- the facade through the same driver
def test_facade_runs_the_reference_sequence(run, tmp_path):
    """tests/cpp/ref_sequence.cpp -- the very source whose run over the reference's files wrote the fixture -- built over the facade
    (cvsteer_amd/facade/Makefile) and run as a child process on the committed inputs: the whole fa:: G2 / G4 surface of the reference,
    protected members included, every plane it writes under the bounds above"""
    planes, points = run
    exe = os.path.join(ROOT, "tests", "cpp", "ref_sequence")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cvsteer_amd", "facade"), "-s"])
    tin, tout = tmp_path / "in", tmp_path / "out"
    tin.mkdir(); tout.mkdir()
    got, got_points = R.run_driver(exe, {n: planes[n] for n in R.INPUTS}, str(tin), str(tout), timeout=120)

    def hold(what, a, b, bound):
        return _hold("facade", what, a, b, bound)

    d_b = 0.0
    for stem, n in (("g2_basis", 7), ("g4_basis", 11), ("g2w3_basis", 7), ("g4w4_basis", 11)):
        for p in range(n):
            name = "%s_%d" % (stem, p)
            d = hold(name, got[name], planes[name], TOL * max(1.0, float(np.abs(planes[name]).max())))
            d_b = max(d_b, d) if stem == "g2_basis" else d_b
    pr = _Prop(planes, d_b)
    for k in (1, 2, 3):
        pr.hold("facade m_c%d" % k, got["g2_c%d" % k], planes["g2_c%d" % k], pr.dC)
    pr.hold("facade strength", got["g2_strength"], planes["g2_strength"], np.sqrt(2) * pr.dC)
    pr.hold_angle("facade theta", got["g2_theta"], planes["g2_theta"], np.pi, pr.dtheta, pr.strong)
    assert (_bits(got["g2_strength"])[pr.zero] == 0).all() and (_bits(got["g2_theta"])[pr.zero] == 0).all()
    for stem, at_theta in (("g2_s0", False), ("g2_s1", False), ("g2_s2", False), ("g2_map", False), ("g2_dom", True)):
        s = _gh_scale(planes[stem + "_g"], planes[stem + "_h"])
        assert np.array_equal(_bits(got[stem + "_g"]), _bits(got[stem + "_g5"])) and np.array_equal(_bits(got[stem + "_h"]), _bits(got[stem + "_h5"]))
        if not at_theta:
            hold(stem + "_g", got[stem + "_g"], planes[stem + "_g"], s)
            hold(stem + "_h", got[stem + "_h"], planes[stem + "_h"], s)
        ok = pr.five("facade " + stem, [got[stem + "_" + x] for x in ("g5", "h5", "e", "mag", "phase")], planes, stem, at_theta)
        if at_theta:
            pr.three("facade find*", [got[n] for n in ("g2_find_edges", "g2_find_dark", "g2_find_bright")], planes, ok)
    for stem in ("g4_s0", "g4_s1", "g4_map"):
        s = _gh_scale(planes[stem + "_g"], planes[stem + "_h"])
        hold(stem + "_g", got[stem + "_g"], planes[stem + "_g"], s)
        hold(stem + "_h", got[stem + "_h"], planes[stem + "_h"], s)
    for stem in ("g2w3", "g4w4"):
        s = _gh_scale(planes[stem + "_g"], planes[stem + "_h"])
        hold(stem + "_g", got[stem + "_g"], planes[stem + "_g"], s)
        hold(stem + "_h", got[stem + "_h"], planes[stem + "_h"], s)
    # the entries that take planes: the bounds of test_entries_that_take_planes
    assert np.allclose(got["craft_mag"], planes["craft_mag"], atol=1e-6, equal_nan=True)
    assert np.array_equal(_bits(got["craft_phase_out"]), _bits(planes["craft_phase_out"]))
    assert np.array_equal(_bits(got["craft_wrap"]), _bits(planes["craft_wrap"]))
    for n in ["craft_pw%d" % k for k in range(5)] + ["craft_edges", "craft_dark", "craft_bright"]:
        hold(n, got[n], planes[n], 1e-6)
    sp = R.phase_specials().size
    for k in range(5):
        n = "craft_pw%d" % k
        assert np.array_equal(_bits(got[n]).flat[:sp] == 0, _bits(planes[n]).flat[:sp] == 0), n      # the gate's side
    # steer(Point): g, h at the steer bound, the rest by the propagation
    bmax = pr.bmax
    for k in range(len(R.THETAS)):
        s = _gh_scale(planes["g2_s%d_g" % k], planes["g2_s%d_h" % k])
        for i in range(len(R.POINTS)):
            w, g = points[k, i], got_points[k, i]
            tag = "point %d at theta %d" % (i, k)
            assert g[0] == g[2] and g[1] == g[3]
            hold(tag + " g", g[2], w[2], s)
            hold(tag + " h", g[3], w[3], s)
            hold(tag + " e", g[4], w[4], 3 * pr.dC)
            hold(tag + " magnitude", g[5], w[5], np.sqrt(2) * 4 * pr.d_b)
            if w[5] > 1e-3 * bmax:
                dp = float(angle_diff(g[6:7], w[6:7], 2 * np.pi)[0])
                assert _note("facade", tag + " phase", dp / (np.sqrt(2) * 4 * pr.d_b / float(w[5]))) <= 1.0


def test_report():
    """the largest fraction of each bound seen by this module's tests (the figures of the docstring)"""
    for stage in sorted(WORST):
        print("largest fraction of the bound, %-14s %.3g" % (stage, WORST[stage]))
    assert all(v <= 1.0 for v in WORST.values())
