"""GPU test (-m gpu): the per-pixel angle math (cvs_device_math.h: sincos_small / sincos_any, angle_0_2pi, and every stage built on
them) held to a plain float64 statement of the same formulas (tests/angle_model.py) on every angle a caller can pass: a dense sweep
of [-8, 8], every multiple of pi / 4 with its ulp neighbours, the reduction's half-way points, both sides of the |x| == 8 switch,
signed zeros, denormals, angles up to FLT_MAX, NaN and +-inf; and for the arctangent every octant boundary with both signs of zero
and magnitudes 2^-40 .. 2^40.  Every plane is 131 x 1021; every test is a handful of launches.

The comparisons are in the project's decoupled-stage form: the basis planes and C1..C3 are read back from the handle and handed to
the model, and the phase of a steer launch is held to the model's arctangent of the g, h that launch stored.  End to end -- against
the arctangent of the model's own g, h -- the distance adds (error of g, h) / magnitude, which the bound on g and h does not keep
under 1e-5 rad at a magnitude of 1e-3: that form is held to 1e-5 + |bound of (g, h)| / magnitude per pixel, and for G2 (where the
measured figure leaves a factor of two) to the plain 1e-5 as well.  The energy of
a steer-by-map call takes 2 theta as the float32 plane of G2.cpp:175: where that overflows (theta = +-FLT_MAX) e is NaN, as at a
non-finite theta.

Bounds: 1e-6 * max(1, sum |plane_i|) per pixel over the planes that enter an output (the stage tolerance of test_gpu_parity.py,
scaled to the plane magnitudes); 1e-5 rad for angles where the magnitude is above 1e-3; 2e-5 for find* on wide phases.

Largest distances (error / bound unless a unit is given)      oracle vs f64 (test_angle_model_cpu.py)      kernel vs f64 (MI355X)
  G2 steer by map  g / h / e / magnitude                        0.14 / 0.18 / 0.11 / 0.16                    0.19 / 0.22 / 0.14 / 0.18
                   phase of the stored g, h                     5.8e-7 rad (end to end 5.1e-6)               5.9e-7 rad (end to end 4.9e-6; G4 extension 8.2e-6)
  G4 steer by map  g / h                                        0.21 / 0.35                                  0.28 / 0.31 (extensions: e 0.16, magnitude 0.21, phase 5.9e-7 rad)
  steering bank    G2 five outputs / G4 g, h                    0.18 / 0.32                                  0.18 / 0.32 (G2 phase 6.1e-7 rad)
  magnitude        |m - hypot| / max(1, hypot)                  8.8e-8                                       1.2e-7
  phase            fastAtan2 polynomial / atan2f                5.8e-7 / 5.1e-7 rad                          5.8e-7 / 4.7e-7 rad; 0 of 976 boundary pairs differ
  phaseWeights / find on unit energy                            3.1e-7 / 3.1e-7                              3.7e-7 / 3.6e-7
  thinning         undecided of 133751 pixels, per map          at most 33                                   at most 32, single and batch launch"""
import numpy as np
import pytest
import torch

import angle_model as A
import cvsteer_amd as cv
from helpers import angle_diff, rand_image
from test_gpu_contours import _check_nms, _random_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-6        # stage tolerance
ANGLE_TOL = 1e-5  # radians, where the vector is longer than MIN_MAG
MIN_MAG = 1e-3
FIND_TOL = 2e-5


def _np(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ratio(got, want, planes, where):
    """largest error / bound over the pixels `where`; a NaN there (a kernel that lost a finite pixel) counts as a miss"""
    r = (np.abs(got - want) / A.bound(planes, TOL))[where]
    assert not np.isnan(r).any(), int(np.isnan(r).sum())
    return float(r.max())


@pytest.fixture(scope="module")
def theta():
    return A.theta_family()


@pytest.fixture(scope="module")
def image():
    return _dev(rand_image(A.ROWS, A.COLS))


def _phase_distances(p, g, h, G, H, bg, bh, ok):
    """(stage form, end to end, end to end / its per-pixel bound): p against the model's arctangent of the stored g, h and of the
    model's G, H; the latter's bound is ANGLE_TOL + |(bound of g, bound of h)| / magnitude"""
    stage = float(angle_diff(p, A.phase(g, h, False), 2 * np.pi)[ok].max())
    e2e = angle_diff(p, A.phase(G, H, False), 2 * np.pi)
    allowed = ANGLE_TOL + np.hypot(A.bound(bg, TOL), A.bound(bh, TOL)) / np.hypot(G, H)
    return stage, float(e2e[ok].max()), float((e2e / allowed)[ok].max())


def _no_neighbour_is_touched(first, steer, theta, fin):
    """the same launch with the non-finite angles replaced by 0.0: every pixel that was finite before keeps its bits"""
    again = [_np(o) for o in steer(_dev(np.where(fin, theta, np.float32(0.0)).astype(np.float32)))]
    for a, b in zip(first, again):
        assert np.array_equal(_bits(a)[fin], _bits(b)[fin])


def test_g2_steer_map_whole_domain(ora, theta, image):
    f = cv.SteerableFiltersG2(image)
    b = [_np(f.basis(p)) for p in range(7)]
    c = [_np(x) for x in f.coefficients()]
    dth = _dev(theta)
    g2, h2 = (_np(o) for o in f.steer(dth))
    outs = [_np(o) for o in f.steer(dth, full=True)]
    g, h, e, m, p = outs
    assert np.array_equal(_bits(g2), _bits(g)) and np.array_equal(_bits(h2), _bits(h))
    t2 = A.two_theta_f32(theta)
    fin = np.isfinite(theta)
    fin_e = fin & np.isfinite(t2)
    G, H, E, M = A.g2_full(b, c, theta, t2)
    r = (_ratio(g, G, b[:3], fin), _ratio(h, H, b[3:], fin), _ratio(e, E, c, fin_e), _ratio(m, M, b, fin))
    ok = fin & (M > MIN_MAG)
    dp, dp_e2e, rp_e2e = _phase_distances(p, g, h, G, H, b[:3], b[3:], ok)
    print("kernel vs f64, G2 steer by map: error / bound g %.3g h %.3g e %.3g magnitude %.3g, phase %.3g rad (end to end %.3g)"
          % (r + (dp, dp_e2e)))
    assert max(r) <= 1.0 and dp <= ANGLE_TOL and dp_e2e <= ANGLE_TOL and rp_e2e <= 1.0
    # NaN / +-inf theta (and e where 2 theta overflows): NaN, and a phase of +0.0 -- the oracle's values
    want = ora.g2_steer_map(np.stack(b), theta, c)
    for got, w in zip(outs, want):
        assert np.array_equal(got[~fin], w[~fin], equal_nan=True)
    assert np.isnan(np.stack(outs[:4])[:, ~fin]).all() and (_bits(p)[~fin] == 0).all()
    assert np.array_equal(e[~fin_e], want[2][~fin_e], equal_nan=True) and np.isnan(e[~fin_e]).all()
    _no_neighbour_is_touched(outs, lambda t: f.steer(t, full=True), theta, fin)


def test_g4_steer_map_whole_domain(ora, theta, image):
    fin = np.isfinite(theta)
    dth = _dev(theta)
    f = cv.SteerableFiltersG4(image)
    b = [_np(f.basis(p)) for p in range(11)]
    g, h = (_np(o) for o in f.steer(dth))
    G, H = A.g4_steer(b, theta)
    r = (_ratio(g, G, b[:5], fin), _ratio(h, H, b[5:], fin))
    print("kernel vs f64, G4 steer by map: error / bound g %.3g h %.3g" % r)
    assert max(r) <= 1.0
    og, oh = ora.g4_steer_map(np.stack(b), theta)
    assert np.array_equal(g[~fin], og[~fin], equal_nan=True) and np.array_equal(h[~fin], oh[~fin], equal_nan=True)
    assert np.isnan(g[~fin]).all() and np.isnan(h[~fin]).all()
    _no_neighbour_is_touched([g, h], f.steer, theta, fin)
    # the extension's five outputs
    fx = cv.SteerableFiltersG4(image, extensions=True)
    bx = [_np(fx.basis(p)) for p in range(11)]
    cx = [_np(x) for x in fx.coefficients()]
    outs = [_np(o) for o in fx.steer(dth, full=True)]
    g, h, e, m, p = outs
    t2 = A.two_theta_f32(theta)
    fin_e = fin & np.isfinite(t2)
    G, H = A.g4_steer(bx, theta)
    E, M = A.energy(cx, theta, t2), np.hypot(G, H)
    r = (_ratio(g, G, bx[:5], fin), _ratio(h, H, bx[5:], fin), _ratio(e, E, cx, fin_e), _ratio(m, M, bx, fin))
    ok = fin & (M > MIN_MAG)
    dp, dp_e2e, rp_e2e = _phase_distances(p, g, h, G, H, bx[:5], bx[5:], ok)
    print("kernel vs f64, G4 steer by map, extensions: error / bound g %.3g h %.3g e %.3g magnitude %.3g, phase %.3g rad (end to end %.3g)"
          % (r + (dp, dp_e2e)))
    assert max(r) <= 1.0 and dp <= ANGLE_TOL and rp_e2e <= 1.0
    assert np.isnan(np.stack(outs[:4])[:, ~fin]).all() and (_bits(p)[~fin] == 0).all() and np.isnan(e[~fin_e]).all()
    _no_neighbour_is_touched(outs, lambda t: fx.steer(t, full=True), theta, fin)


def test_steer_bank_whole_domain(image):
    angles = A.bank_angles()
    assert angles.size > 3 * 32   # kBankMax = 32 angles per launch: four launches
    everywhere = np.ones((A.ROWS, A.COLS), bool)
    f = cv.SteerableFiltersG2(image)
    b = [_np(f.basis(p)) for p in range(7)]
    c = [_np(x) for x in f.coefficients()]
    bank = f.steer_bank(angles, full=True)
    worst, worst_p = 0.0, 0.0
    for k, t in enumerate(angles):
        one = f.steer(float(t), full=True)
        for kind in range(5):
            assert torch.equal(bank[kind][k].view(torch.int32), one[kind].view(torch.int32)), (kind, k, float(t))
        g, h, e, m, p = (_np(bank[kind][k]) for kind in range(5))
        G, H, E, M = A.g2_full(b, c, t)
        worst = max(worst, _ratio(g, G, b[:3], everywhere), _ratio(h, H, b[3:], everywhere), _ratio(e, E, c, everywhere),
                    _ratio(m, M, b, everywhere))
        worst_p = max(worst_p, float(angle_diff(p, A.phase(g, h, False), 2 * np.pi)[M > MIN_MAG].max()))
    f4 = cv.SteerableFiltersG4(image)
    b4 = [_np(f4.basis(p)) for p in range(11)]
    bank4 = f4.steer_bank(angles)
    worst4 = 0.0
    for k, t in enumerate(angles):
        one = f4.steer(float(t))
        for kind in range(2):
            assert torch.equal(bank4[kind][k].view(torch.int32), one[kind].view(torch.int32)), (kind, k, float(t))
        G, H = A.g4_steer(b4, t)
        worst4 = max(worst4, _ratio(_np(bank4[0][k]), G, b4[:5], everywhere), _ratio(_np(bank4[1][k]), H, b4[5:], everywhere))
    print("kernel vs f64, steering bank at %d angles: error / bound G2 %.3g, G4 %.3g, G2 phase %.3g rad" % (angles.size, worst, worst4, worst_p))
    assert worst <= 1.0 and worst4 <= 1.0 and worst_p <= ANGLE_TOL


@pytest.mark.parametrize("exact", [False, True])
def test_mag_phase_whole_domain(ora, exact):
    g, h, boundary = A.gh_family()
    f = cv.SteerableFiltersG2(None)
    f.set_atan_mode(exact)
    m, p = (_np(o) for o in f.computeMagnitudeAndPhase(_dev(g), _dev(h)))
    hyp = np.hypot(g.astype(np.float64), h.astype(np.float64))
    dm = float((np.abs(m - hyp) / np.maximum(1.0, hyp)).max())
    dp = float(angle_diff(p, A.phase(g, h, exact), 2 * np.pi).max())
    _, op = ora.mag_phase(g, h, ora.ATAN_EXACT if exact else ora.ATAN_CV)
    differ = int(np.count_nonzero(_bits(p)[boundary] != _bits(op)[boundary]))
    print("kernel vs f64, magnitude / phase (exact=%s): magnitude %.3g max(1, hypot), phase %.3g rad; %d of %d boundary pairs differ "
          "from the oracle's bits" % (exact, dm, dp, differ, int(boundary.sum())))
    assert dm <= TOL and dp <= ANGLE_TOL
    # diagonals, axes, zeros of either sign: the branch is an exact comparison of the inputs, so the phase is the oracle's, bit for bit
    assert differ == 0


def test_phase_weights_whole_domain(theta):
    fin = np.isfinite(theta)
    f = cv.SteerableFiltersG2(None)
    dth = _dev(theta)
    worst = 0.0
    for phi in A.PHIS:
        for signum in (False, True):
            lam = _np(f.phaseWeights(dth, phi, signum))
            d = np.abs(lam - A.phase_weights(theta, phi, signum))[fin]
            assert not np.isnan(d).any(), (phi, signum)
            worst = max(worst, float(d.max()))
            assert worst <= TOL, (phi, signum, worst)
    ones = torch.ones((A.ROWS, A.COLS), device=DEV)
    dfind = 0.0
    for got, want in zip(f.find(ones, dth), A.find_weights(theta)):
        d = np.abs(_np(got) - want)[fin]
        assert not np.isnan(d).any()
        dfind = max(dfind, float(d.max()))
    print("kernel vs f64, phaseWeights %.3g, find on unit energy %.3g" % (worst, dfind))
    assert dfind <= FIND_TOL


def test_nonmax_theta_whole_domain(image):
    f = cv.SteerableFiltersG2(image)
    thetas = A.nms_thetas()
    cases = [_random_case(A.ROWS, A.COLS, seed)[0] for seed in A.NMS_SEEDS]
    singles = []
    for maps, th in zip(cases, thetas):
        got = f.nonmax([_dev(m) for m in maps], theta=_dev(th))
        for g, m in zip(got, maps):
            _check_nms(g, m, th)
            assert (_bits(_np(g))[~np.isfinite(th)] == 0).all()   # a non-finite theta stores +0.0
        singles.append(torch.stack(list(got)))
    # the same two frames through the batch launch
    block = _dev(np.stack([np.stack(maps) for maps in cases]))
    got = f.nonmax_batch(block, theta=_dev(np.stack(thetas)))
    assert torch.equal(got.view(torch.int32), torch.stack(singles).view(torch.int32))
    for i, (maps, th) in enumerate(zip(cases, thetas)):
        for k, m in enumerate(maps):
            _check_nms(got[i, k], m, th)
            assert (_bits(_np(got[i, k]))[~np.isfinite(th)] == 0).all()
