"""The float64 angle model (angle_model.py) and its input families, checked without a GPU: the oracle's float32 restatement of every
per-pixel stage is run on the families and held to the model at the very bounds tests/test_gpu_angle_domain.py asks of the
kernels, so the reference alone is shown to fit them; the thinning families are shown to stay under the undecided cap from the model
alone; and the families are shown to contain what they promise.

Largest distances, oracle vs f64 (this module prints them; `bound` is 1e-6 * max(1, sum |plane_i|) per pixel, angle_model.bound):
  G2 steer by map     g 0.14 bound (2.1e-7)   h 0.18 bound (3.1e-7)   e 0.11 bound (2.6e-7)   magnitude 0.16 bound (3.4e-7)
                      phase of the oracle's own g, h 5.8e-7 rad where magnitude > 1e-3 (end to end 5.1e-6 rad)
  G4 steer by map     g 0.21 bound            h 0.35 bound
  scalar steer at the bank's 100 angles        G2 g, h, e, magnitude 0.18 bound    G4 g, h 0.32 bound
  magnitude / phase   |m - hypot| 8.8e-8 max(1, hypot)   phase 5.8e-7 rad (fastAtan2 polynomial)   5.1e-7 rad (atan2f)
  phaseWeights        3.1e-7 over the eight phi and both signum      find on unit energy 3.1e-7
  thinning            at most 33 of 133751 pixels undecided per map (cap 1e-3: 133)"""
import numpy as np
import pytest

import angle_model as A
import contour_model as M
from helpers import angle_diff, rand_image

TOL = 1e-6        # the stage tolerance (tests/test_gpu_parity.py header)
ANGLE_TOL = 1e-5  # the angle tolerance, radians
FIND_TOL = 2e-5   # what the suite gives find* on wide phases
UNDECIDED = 1e-3  # _check_nms' cap


@pytest.fixture(scope="module")
def theta():
    return A.theta_family()


@pytest.fixture(scope="module")
def g2_planes(ora):
    b = ora.basis(ora.KIND_G2, rand_image(A.ROWS, A.COLS), 4, 0.67)
    return b, ora.g2_orientation(b)[:3]


@pytest.fixture(scope="module")
def g4_planes(ora):
    return ora.basis(ora.KIND_G4, rand_image(A.ROWS, A.COLS), 6, 0.5)


def _ratio(got, want, planes, where):
    return float((np.abs(got - want) / A.bound(planes, TOL))[where].max())


def test_families_hold_what_they_promise(theta):
    assert theta.shape == (A.ROWS, A.COLS) and theta.dtype == np.float32
    assert np.array_equal(theta, A.theta_family(), equal_nan=True)   # a pure function of the seed
    flat = theta.ravel()
    bits = set(flat.view(np.uint32).tolist())

    def has(v):
        return int(np.float32(v).view(np.uint32)) in bits

    f8 = np.float32(8.0)
    for v in (8.0, -8.0, np.nextafter(f8, np.float32(0)), np.nextafter(-f8, np.float32(0)), np.nextafter(f8, np.float32(np.inf)),
              np.nextafter(-f8, np.float32(-np.inf)), 0.0, -0.0, 1e-40, -1e-40, 1e-20, -1e-20, np.inf, -np.inf):
        assert has(v), v
    assert np.float32(1e-40) != 0 and abs(float(np.float32(1e-40))) < float(np.finfo(np.float32).tiny)   # a denormal
    assert np.isnan(flat).sum() >= 1
    for v in A.LARGE:
        assert has(v) and has(-v), v
    for n in range(-10, 11):       # every multiple of pi / 4 up to 8, with its +-1..4 ulp neighbours
        for w in A._steps([np.float32(n * np.pi / 4)], 4):
            assert has(w), (n, w)
    # the reduction's half-way points: k = rint(x * 2/pi) is decided at a product of exactly n + 1/2, and both sides are present
    prod = (flat * A.K_TWO_OVER_PI).astype(np.float32)
    for n in range(-5, 5):
        x0 = (n + 0.5) * np.pi / 2
        near = np.abs(flat.astype(np.float64) - x0) < 1e-5
        assert (prod[near] <= n + 0.5).any() and (prod[near] >= n + 0.5).any(), n
        for w in A._steps([np.float32(x0)], 1):
            assert has(w)
    # k = rint(x * 2/pi) reaches +-4 and +-5 below |x| = 8, and every quadrant of both signs is there
    k = np.rint(prod[np.abs(flat) <= 8])
    assert set(range(-5, 6)) <= set(k.astype(int).tolist())
    for d in range(1, 8):          # each decade from 10 to 1e8
        a = np.abs(flat)
        assert ((a >= 10.0 ** d) & (a < 10.0 ** (d + 1))).sum() >= A.N_DECADE
    sweep = flat[:A.N_SWEEP]
    assert sweep[0] == -8 and sweep[-1] == 8 and np.diff(sweep).max() < 2e-4
    assert np.isfinite(flat).sum() == flat.size - A.NONFINITE_TAIL.size
    # the bank's angles: special values only, more than one launch of kBankMax = 32 angles
    ang = A.bank_angles()
    assert ang.size == 100 and np.isfinite(ang).all() and np.isin(ang, A.theta_special()).all()
    for v in (8.0, -8.0, np.nextafter(f8, np.float32(np.inf)), 0.0, 1e-40, 1e30, A.FLT_MAX, -A.FLT_MAX):
        assert np.float32(v) in ang


def test_gh_family_holds_what_it_promises():
    g, h, bd = A.gh_family()
    assert g.shape == h.shape == bd.shape == (A.ROWS, A.COLS) and g.dtype == h.dtype == np.float32
    ag, ah = np.abs(g), np.abs(h)
    assert ((ag == ah) | (g == 0) | (h == 0))[bd].all()
    pairs = set(zip(g[bd].view(np.uint32).tolist(), h[bd].view(np.uint32).tolist()))
    u = lambda v: int(np.float32(v).view(np.uint32))
    for k in (-40, -1, 0, 1, 40):
        m = 2.0 ** k
        for a in (m, -m):
            for b in (m, -m):
                assert (u(a), u(b)) in pairs                 # the four diagonals
            for z in (0.0, -0.0):
                assert (u(a), u(z)) in pairs and (u(z), u(a)) in pairs   # the axes, both signs of the zero
    for a in (0.0, -0.0):
        for b in (0.0, -0.0):
            assert (u(a), u(b)) in pairs
    # every octant, the ratio min / max dense over [0, 1] in each, every magnitude 2^-40 .. 2^40
    rest = ~bd
    with np.errstate(all="ignore"):
        ratio = np.minimum(ag, ah) / np.maximum(ag, ah)
    for x_major in (True, False):
        for sx in (False, True):
            for sy in (False, True):
                o = rest & ((ag >= ah) == x_major) & (np.signbit(g) == sx) & (np.signbit(h) == sy)
                r = np.sort(ratio[o & (ratio > 0) & (ratio < 1)])
                assert r.size > 10000 and r[0] < 1e-3 and r[-1] > 0.999 and np.diff(r).max() < 1e-3
    assert set(np.log2(np.maximum(ag, ah)[rest & (np.maximum(ag, ah) > 0)]).round().astype(int).tolist()) >= set(A.GH_EXPONENTS)
    sq = (g * g + h * h)[(g != 0) | (h != 0)]
    assert np.isfinite(sq).all() and sq.min() >= np.finfo(np.float32).tiny   # g^2 + h^2 stays normal


def test_oracle_g2_steer_map_fits_the_bound(ora, theta, g2_planes):
    b, c = g2_planes
    og, oh, oe, om, op = ora.g2_steer_map(b, theta, c)
    g, h, e, m = A.g2_full(b, c, theta, A.two_theta_f32(theta))
    fin = np.isfinite(theta)
    fin_e = fin & np.isfinite(A.two_theta_f32(theta))   # 2 theta overflows float32 at +-FLT_MAX: no energy there (angle_model)
    assert fin.sum() - fin_e.sum() == 2
    r = {"g": _ratio(og, g, b[:3], fin), "h": _ratio(oh, h, b[3:], fin), "e": _ratio(oe, e, c, fin_e), "magnitude": _ratio(om, m, b, fin)}
    # the phase in the decoupled-stage form -- the model's arctangent of the very g, h the stage was handed -- and end to end, where
    # the distance adds (error of g, h) / magnitude (tests/test_gpu_angle_domain.py holds G2 to the plain 1e-5 in that form too)
    ok = fin & (m > 1e-3)
    dp = float(angle_diff(op, A.phase(og, oh, False), 2 * np.pi)[ok].max())
    dp_e2e = float(angle_diff(op, A.phase(g, h, False), 2 * np.pi)[ok].max())
    print("oracle vs f64, G2 steer by map: error / bound %s, phase %.3g rad (end to end %.3g)" % (r, dp, dp_e2e))
    assert max(r.values()) <= 1.0 and dp <= ANGLE_TOL and dp_e2e <= ANGLE_TOL
    # non-finite theta: NaN everywhere but the phase, which patchNaNs makes 0.0
    for o in (og, oh, oe, om):
        assert np.isnan(o[~fin]).all()
    assert np.isnan(oe[~fin_e]).all() and (op[~fin].view(np.uint32) == 0).all()


def test_oracle_g4_steer_map_fits_the_bound(ora, theta, g4_planes):
    b = g4_planes
    og, oh = ora.g4_steer_map(b, theta)
    g, h = A.g4_steer(b, theta)
    fin = np.isfinite(theta)
    r = {"g": _ratio(og, g, b[:5], fin), "h": _ratio(oh, h, b[5:], fin)}
    print("oracle vs f64, G4 steer by map: error / bound %s" % r)
    assert max(r.values()) <= 1.0
    assert np.isnan(og[~fin]).all() and np.isnan(oh[~fin]).all()


def test_oracle_scalar_steer_at_the_bank_angles_fits_the_bound(ora, g2_planes, g4_planes):
    b, c = g2_planes
    worst2 = worst4 = 0.0
    everywhere = np.ones(b[0].shape, bool)
    for t in A.bank_angles():
        og, oh, oe, om, _ = ora.g2_steer_scalar(b, float(t), c)
        g, h, e, m = A.g2_full(b, c, t)
        worst2 = max(worst2, _ratio(og, g, b[:3], everywhere), _ratio(oh, h, b[3:], everywhere), _ratio(oe, e, c, everywhere),
                     _ratio(om, m, b, everywhere))
        og, oh = ora.g4_steer_scalar(g4_planes, float(t))
        g, h = A.g4_steer(g4_planes, t)
        worst4 = max(worst4, _ratio(og, g, g4_planes[:5], everywhere), _ratio(oh, h, g4_planes[5:], everywhere))
    print("oracle vs f64, scalar steer at the bank's angles: error / bound G2 %.3g, G4 %.3g" % (worst2, worst4))
    assert worst2 <= 1.0 and worst4 <= 1.0


@pytest.mark.parametrize("exact", [False, True])
def test_oracle_mag_phase_fits_the_bound(ora, exact):
    g, h, _ = A.gh_family()
    om, op = ora.mag_phase(g, h, ora.ATAN_EXACT if exact else ora.ATAN_CV)
    hyp = np.hypot(g.astype(np.float64), h.astype(np.float64))
    dm = float((np.abs(om - hyp) / np.maximum(1.0, hyp)).max())
    dp = float(angle_diff(op, A.phase(g, h, exact), 2 * np.pi).max())
    print("oracle vs f64, magnitude / phase (exact=%s): magnitude %.3g max(1, hypot), phase %.3g rad" % (exact, dm, dp))
    assert dm <= TOL and dp <= ANGLE_TOL


def test_oracle_phase_weights_fit_the_bound(ora, theta):
    fin = np.isfinite(theta)
    worst = 0.0
    for phi in A.PHIS:
        for signum in (False, True):
            d = np.abs(ora.phase_weights(theta, phi, signum) - A.phase_weights(theta, phi, signum))[fin].max()
            worst = max(worst, float(d))
    ones = np.ones_like(theta)
    dfind = max(float(np.abs(o - w)[fin].max()) for o, w in zip(ora.find(ones, theta), A.find_weights(theta)))
    print("oracle vs f64, phaseWeights %.3g, find on unit energy %.3g" % (worst, dfind))
    assert worst <= TOL and dfind <= FIND_TOL


def test_thinning_family_stays_under_the_undecided_cap():
    """what tests/test_gpu_angle_domain.py hands to _check_nms: the share of pixels the model itself calls undecided"""
    from test_gpu_contours import _random_case   # the maps the thinning tests use (needs no GPU to draw them)
    for seed, th in zip(A.NMS_SEEDS, A.nms_thetas()):
        maps, _ = _random_case(A.ROWS, A.COLS, seed)
        c, s = M.directions(th)
        for m in maps:
            _, vb, vf = M.nonmax_parts(m, c, s)
            und = int(np.count_nonzero(~M.decided(m, vb, vf)))
            print("thinning family, seed %d: %d of %d undecided" % (seed, und, m.size))
            assert und < UNDECIDED * m.size
