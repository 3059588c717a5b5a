"""The oracle, and the float64 models, held to planes that the REFERENCE'S OWN source files wrote (tests/golden/ref_run/, made by
oracle/ref_run.mk: the reference's three .cpp files compiled where they lie over the stand-in headers of oracle/cvshim, driven by
tests/cpp/ref_sequence.cpp).  The oracle and the kernels were both written from one reading of that source; a slip made in the
reading -- a coefficient of C1..C3, the pairing of a tap vector with a basis plane, a steering sign, a gate -- is in both and only data
the reference itself produced can show it.  No GPU here.

Every oracle function is fed the fixture's own upstream planes (decoupled stages) and held to the fixture's output at
1e-6 * max(1, largest |term| of the stage); angles modulo their cut at 5e-6 rad on every pixel.  What is recalled rather than pinned
are the stand-in's OpenCV primitives (sepFilter2D, cartToPolar, polarToCart are the oracle's own C functions; operators are eager, one
float32 plane each; double scalars narrowed to float): where the oracle folds a scalar into a sum as OpenCV's MatExpr does, the eager
stand-in adds in another order and the two differ by an ulp.

Measured, oracle vs reference run (this module prints them; distance / bound):
  BIT FOR BIT   basis G2 (4, 0.67), (3, 0.9), G4 (6, 0.5), (4, 0.75); G2 steer(theta) g, h, e, magnitude, phase at the three angles;
                G2 steer(map) g and e at both maps, magnitude and phase of the run's own g, h; strength and theta of the run's own
                C2, C3; steer(Point) g, h, e, magnitude, phase at 7 points x 3 angles; computeMagnitudeAndPhase, wrap, the five
                phaseWeights and the three find* on the crafted planes, find* on the image; G4 steer(theta) and steer(map) g, h
  C1 0.101   C2 0.076   C3 0.186   strength 0.128   theta 2.8e-7 rad         (one ulp of the largest term: the eager sums)
  steer(map) h 0.077 / 0.089 (dominant / random map)   magnitude 0.056 / 0.058   phase 4.8e-7 / 9.5e-7 rad (from the oracle's own h)
Known answers (taps_ref.json, kernel pairs) vs the run's basis planes: at most 2.3e-7 of max|plane| (bound 1e-5).  The float64 models vs
the run: C1..C3 0.047 / 0.065 / 0.025 of orientation_model.bound, strength 0.097, theta 2.7e-7 rad; phaseWeights and find 2.8e-7; steer
g, h, e at most 0.16 (G2) and 0.23 (G4) of angle_model.bound, magnitude 9.4e-8, phase 5.6e-7 rad.
The teeth (mutations applied in the test to the oracle's inputs or outputs; excess over the stage bound): h2b / h2c swapped 1.4e6 x,
H bank negated 2.9e6 x, g4b / g4d swapped 1.4e6 x, C3's 1.6875 -> 1.5 2.8e4 x.  The phaseWeights gate at >= instead of > differs from >
only where the folded error is exactly float(pi / 2) -- 11 pixels of the crafted plane -- and there by cos^2(float(pi / 2)) = 1.9e-15,
nine orders below the stage bound: no distance can give that mutation a factor of 100, so the gate's side is asserted bit for bit on
those pixels instead (test_teeth_phase_weights_gate)."""
import os

import numpy as np
import pytest

import angle_model as A
import known_answers as K
import orientation_model as O
import ref_run_fixture as R
from helpers import angle_diff

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_RUN = os.path.join(ROOT, "oracle", "_ref", "ref_run")
TOL = 1e-6          # the decoupled-stage tolerance (tests/test_gpu_parity.py header)
ANGLE_TOL = 5e-6    # radians, modulo the cut
TEETH = 100.0       # a mutation must exceed the stage bound by this factor

# C1..C3 as SteerableFiltersG2.cpp:93-95 writes them: coefficient, (i, j) = product of basis planes i and j (g2a g2b g2c h2a h2b h2c h2d)
C_TERMS = {1: [(0.5, 1, 1), (0.25, 0, 2), (0.375, 0, 0), (0.375, 2, 2), (0.3125, 3, 3), (0.3125, 6, 6), (0.5625, 4, 4), (0.5625, 5, 5),
               (0.375, 3, 5), (0.375, 4, 6)],
           2: [(0.5, 0, 0), (-0.5, 2, 2), (0.46875, 3, 3), (-0.46875, 6, 6), (0.28125, 4, 4), (-0.28125, 5, 5), (0.1875, 3, 5), (-0.1875, 4, 6)],
           3: [(-1.0, 0, 1), (-1.0, 1, 2), (-0.9375, 5, 6), (-0.9375, 3, 4), (-1.6875, 4, 5), (-0.1875, 3, 6)]}


@pytest.fixture(scope="module")
def run(golden_dir):
    """the committed planes and point values: loaded once, left unchanged"""
    planes, points = R.load(golden_dir)
    for p in planes.values():
        p.setflags(write=False)
    return planes, points


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _bound(*terms):
    """1e-6 * max(1, largest |term| of the stage), one number per stage; non-finite terms (the crafted NaN / Inf) do not count"""
    m = 1.0
    for t in terms:
        t = np.abs(np.asarray(t, F64))
        t = t[np.isfinite(t)]
        if t.size:
            m = max(m, float(t.max()))
    return TOL * m


def _dist(got, want):
    """largest |got - want| over the pixels where either is finite; a NaN or an infinity must sit in the same place on both sides"""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    fin = np.isfinite(got) & np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True)
    return float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0


SEEN = {}


def _hold(name, got, want, bound, exact=False):
    d = _dist(got, want)
    SEEN[name] = (d / bound, _same(got, want))
    print("oracle vs reference run, %-28s %.3g of the bound%s" % (name, d / bound, "  (bit for bit)" if _same(got, want) else ""))
    assert d <= bound, (name, d, bound)
    if exact:
        assert _same(got, want), name


def _hold_angle(name, got, want, period, exact=False):
    d = float(angle_diff(np.asarray(got), np.asarray(want), period).max())
    if period == np.pi:
        d = float(O.theta_error(got, want).max())
    print("oracle vs reference run, %-28s %.3g rad%s" % (name, d, "  (bit for bit)" if _same(got, want) else ""))
    assert d <= ANGLE_TOL, (name, d)
    if exact:
        assert _same(got, want), name


def _stack(planes, stem, n):
    return np.stack([planes["%s_%d" % (stem, i)] for i in range(n)])


def _g2_weights(theta):
    c, s = np.cos(F64(theta)), np.sin(F64(theta))
    return [c * c, -2 * c * s, s * s, c ** 3, -3 * c * c * s, 3 * c * s * s, -s ** 3]


def _steer_terms(b, weights):
    return [np.asarray(w, F64) * b[i].astype(F64) for i, w in enumerate(weights)]


# ---- regeneration ----
def test_reference_run_regenerates_the_fixture_byte_for_byte(run, tmp_path):
    """where oracle/_ref/ref_run exists (build() makes it wherever the reference's sources are), running it on the committed inputs
    gives every committed plane again, byte for byte, and the numpy inputs and the index are what ref_run_fixture makes"""
    if not os.path.exists(REF_RUN):
        pytest.skip("oracle/_ref/ref_run is not built: the reference's sources are not on this machine (oracle/ref_run.mk needs them)")
    planes, points = run
    tin, tout = tmp_path / "in", tmp_path / "out"
    tin.mkdir(); tout.mkdir()
    got, got_points = R.run_driver(REF_RUN, {n: planes[n] for n in R.INPUTS}, str(tin), str(tout))
    assert sorted(got) == sorted(R.OUTPUT_PLANES)
    for n in R.OUTPUT_PLANES:
        assert got[n].tobytes() == planes[n].tobytes(), n
    assert got_points.tobytes() == points.tobytes()


def test_fixture_holds_what_it_promises(run, golden_dir):
    import json
    planes, points = run
    made = R.make_inputs()
    for n in R.INPUTS:
        assert made[n].tobytes() == planes[n].tobytes(), n      # the inputs are a pure function of the seed
    d = R.golden_ref_run(golden_dir)
    assert json.load(open(os.path.join(d, "index.json"))) == json.loads(json.dumps(R.index()))
    assert sorted(os.listdir(d)) == sorted([f + ".npy" for f in R.FILES] + [R.POINTS_FILE + ".npy", "index.json"])
    assert all(os.path.getsize(os.path.join(d, f)) <= R.MAX_FILE_BYTES for f in os.listdir(d))
    img = planes["image"]
    assert img.shape == (24, 70) and (img[-R.ZERO_ROWS:] == 0).all() and R.ZERO_ROWS >= 6
    assert np.array_equal(img, img.astype(np.uint8).astype(F32)) and img.max() > 200           # whole byte values: a byte image holds it
    zero = slice(24 - R.ZERO_ROWS + 4, 24)                                                       # beyond the reach of 9 taps
    c2, c3, th, st = (planes[k] for k in ("g2_c2", "g2_c3", "g2_theta", "g2_strength"))
    assert (_bits(c2[zero]) == 0).all() and (c3[zero] == 0).all()                                # exact (C2, C3) = (0, 0)
    assert (_bits(st[zero]) == 0).all() and (_bits(th[zero]) == 0).all()                         # +0 strength, theta 0
    live = st[:24 - R.ZERO_ROWS - 4]
    assert (live > 1e-3 * live.max()).mean() > 0.5                                               # a well-conditioned part
    tm = planes["theta_map"]
    assert np.abs(tm).max() < np.pi / 2 and tm.min() < -1.5 and tm.max() > 1.5
    g, h = planes["craft_g"], planes["craft_h"]
    sp = R.pair_specials()
    assert _same(g.flat[:len(sp)], sp[:, 0]) and _same(h.flat[:len(sp)], sp[:, 1])
    pairs = set(zip(_bits(g).ravel().tolist(), _bits(h).ravel().tolist()))
    u = lambda v: int(_bits(np.array([v], F32))[0])
    for z in (0.0, -0.0):
        for a in (1.0, -1.0):
            assert (u(a), u(z)) in pairs and (u(z), u(a)) in pairs                               # both axes, either sign of the zero
        for z2 in (0.0, -0.0):
            assert (u(z), u(z2)) in pairs                                                        # (0, 0)
    assert np.isnan(g).sum() == 1 and np.isinf(g).sum() == 1
    m = np.hypot(g.astype(F64), h.astype(F64))
    m = m[np.isfinite(m) & (m > 0)]
    assert m.min() <= 2.0 ** -19 and m.max() >= 2.0 ** 20
    ph = planes["craft_phase"]
    assert _same(ph.flat[:18], R.phase_specials()) and np.abs(ph).max() == np.nextafter(R.PI32, F32(4))
    for v in (0.0, R.HALF_PI32, -R.HALF_PI32, R.PI32, -R.PI32):
        for w in (np.nextafter(F32(v), F32(-9)), F32(v), np.nextafter(F32(v), F32(9))):
            assert (ph == w).any(), w
    assert _same(planes["craft_angle"].flat[:9], R.angle_specials())
    assert points.shape == (3, 7, 7)


# ---- the oracle against the run, stage by stage ----
@pytest.mark.parametrize("tag,kind,cfg,files", [("g2", 2, R.G2_DEFAULT, ("g2_basis",)), ("g4", 4, R.G4_DEFAULT, ("g4_basis",)),
                                                ("g2w3", 2, R.G2_GENERIC, ("g2w3_basis",)), ("g4w4", 4, R.G4_GENERIC, ("g4w4_basis",))])
def test_oracle_basis(ora, run, tag, kind, cfg, files):
    """taps, and the pairing of tap vectors with basis planes, as the reference's constructors and setup() wrote them"""
    planes, _ = run
    want = _stack(planes, files[0], 7 if kind == 2 else 11)
    got = ora.basis(kind, planes["image"], cfg[0], cfg[1])
    _hold("basis " + tag, got, want, _bound(want), exact=True)


def test_oracle_g2_orientation(ora, run):
    planes, _ = run
    b = _stack(planes, "g2_basis", 7)
    c1, c2, c3, th, st = ora.g2_orientation(b)
    b64 = b.astype(F64)
    for k, got in ((1, c1), (2, c2), (3, c3)):
        terms = [c * b64[i] * b64[j] for c, i, j in C_TERMS[k]]
        _hold("C%d" % k, got, planes["g2_c%d" % k], _bound(*terms))
    want_c2, want_c3 = planes["g2_c2"], planes["g2_c3"]
    _hold("strength", st, planes["g2_strength"], _bound(want_c2, want_c3))
    _hold_angle("theta", th, planes["g2_theta"], np.pi)
    # decoupled: the angle and the strength of the fixture's own (C2, C3) through the oracle's cartToPolar / wrap / * 0.5 -- the very
    # functions the stand-in calls, so this pins wrap-then-halve and the argument order, bit for bit
    m, a = ora.cart_to_polar(want_c2, want_c3)
    _hold("strength of own C2, C3", m, planes["g2_strength"], _bound(want_c2, want_c3), exact=True)
    _hold_angle("theta of own C2, C3", (ora.wrap(a) * F32(0.5)).astype(F32), planes["g2_theta"], np.pi, exact=True)


def _hold_steer5(tag, got, planes, stem, b, c, weights, two_theta, h_exact):
    g, h, e, m, p = got
    terms = _steer_terms(b, weights)
    bg, bh = _bound(*terms[:3]), _bound(*terms[3:])
    for suffix in ("", "5"):        # the two-output form and the five-output form of the reference give the same g, h
        _hold("%s g%s" % (tag, suffix), g, planes[stem + "_g" + suffix], bg, exact=True)
        _hold("%s h%s" % (tag, suffix), h, planes[stem + "_h" + suffix], bh, exact=h_exact)
    c64 = [x.astype(F64) for x in c]
    _hold(tag + " e", e, planes[stem + "_e"], _bound(c64[0], c64[1] * np.cos(two_theta), c64[2] * np.sin(two_theta)), exact=True)
    return planes[stem + "_g5"], planes[stem + "_h5"], m, p


def _coeffs(planes):
    return planes["g2_c1"], planes["g2_c2"], planes["g2_c3"]


@pytest.mark.parametrize("k", [0, 1, 2])
def test_oracle_g2_steer_scalar(ora, run, k):
    planes, _ = run
    b, c, theta, stem = _stack(planes, "g2_basis", 7), _coeffs(planes), R.THETAS[k], "g2_s%d" % k
    got = ora.g2_steer_scalar(b, theta, c)
    wg, wh, m, p = _hold_steer5("steer(%.2f)" % theta, got, planes, stem, b, c, _g2_weights(theta), 2.0 * F64(theta), True)
    _hold("steer(%.2f) magnitude" % theta, m, planes[stem + "_mag"], _bound(wg, wh), exact=True)
    _hold_angle("steer(%.2f) phase" % theta, p, planes[stem + "_phase"], 2 * np.pi, exact=True)
    g2, h2 = ora.g2_steer_scalar(b, theta)
    assert _same(g2, got[0]) and _same(h2, got[1])


@pytest.mark.parametrize("stem,theta_name", [("g2_dom", "g2_theta"), ("g2_map", "theta_map")])
def test_oracle_g2_steer_map(ora, run, stem, theta_name):
    planes, _ = run
    b, c, theta = _stack(planes, "g2_basis", 7), _coeffs(planes), planes[theta_name]
    got = ora.g2_steer_map(b, theta, c)
    wg, wh, m, p = _hold_steer5("steer(%s)" % theta_name, got, planes, stem, b, c, _g2_weights(theta), A.two_theta_f32(theta), False)
    # decoupled: magnitude and phase from the fixture's own g, h are the oracle's bit for bit; from the oracle's g, h within the bound
    dm, dp = ora.mag_phase(wg, wh)
    _hold("steer(%s) magnitude of own g, h" % theta_name, dm, planes[stem + "_mag"], _bound(wg, wh), exact=True)
    _hold_angle("steer(%s) phase of own g, h" % theta_name, dp, planes[stem + "_phase"], 2 * np.pi, exact=True)
    _hold("steer(%s) magnitude" % theta_name, m, planes[stem + "_mag"], _bound(wg, wh))
    ok = planes[stem + "_mag"] > 1e-3      # the phase of the oracle's own g, h moves with them where the magnitude is tiny
    _hold_angle("steer(%s) phase" % theta_name, np.where(ok, p, 0), np.where(ok, planes[stem + "_phase"], 0), 2 * np.pi)


def test_oracle_g2_steer_point(ora, run):
    planes, points = run
    b, c = _stack(planes, "g2_basis", 7), _coeffs(planes)
    bmax = [float(np.abs(x).max()) for x in b]
    for k, theta in enumerate(R.THETAS):
        w = _g2_weights(theta)
        for i, (x, y) in enumerate(R.POINTS):
            got = ora.g2_steer_point(b, c, y, x, theta)
            want = points[k, i]
            tg = [w[j] * F64(b[j][y, x]) for j in range(3)]
            th = [w[j] * F64(b[j][y, x]) for j in range(3, 7)]
            tag = "point (%d, %d) at %.2f" % (x, y, theta)
            assert _same(want[0], want[2]) and _same(want[1], want[3]), tag      # the two forms of the reference agree
            _hold(tag + " g", got[0:1], want[0:1], _bound(*tg), exact=True)
            _hold(tag + " h", got[1:2], want[1:2], _bound(*th), exact=True)
            _hold(tag + " e", got[2:3], want[4:5], _bound(*[x_[y, x] for x_ in c]), exact=True)
            _hold(tag + " magnitude", got[3:4], want[5:6], _bound(want[2], want[3]), exact=True)
            _hold_angle(tag + " phase", got[4:5], want[6:7], 2 * np.pi, exact=True)
    assert (points[:, 2:4, :] == 0).all()      # the two bottom corners lie in the zero band


def test_oracle_mag_phase_wrap_on_the_crafted_planes(ora, run):
    planes, _ = run
    g, h = planes["craft_g"], planes["craft_h"]
    m, p = ora.mag_phase(g, h)
    _hold("crafted magnitude", m, planes["craft_mag"], _bound(g, h), exact=True)
    _hold_angle("crafted phase", p, planes["craft_phase_out"], 2 * np.pi, exact=True)
    nan = np.isnan(g) | np.isnan(h)
    assert nan.sum() == 1 and (_bits(planes["craft_phase_out"])[nan] == 0).all()        # patchNaNs
    assert np.isfinite(planes["craft_phase_out"]).all()
    _hold("wrap", ora.wrap(planes["craft_angle"]), planes["craft_wrap"], _bound(planes["craft_angle"]), exact=True)
    a = planes["craft_angle"]
    assert _same(planes["craft_wrap"], np.where(a > R.PI32, a - R.TWO_PI32, a))        # the definition itself, narrowed scalars


def test_oracle_phase_weights_and_find(ora, run):
    planes, _ = run
    ph = planes["craft_phase"]
    for k, (phi, signum) in enumerate(R.PHASE_WEIGHTS):
        _hold("phaseWeights(%.2f, %s)" % (phi, signum), ora.phase_weights(ph, phi, signum), planes["craft_pw%d" % k], TOL, exact=True)
    ones = np.ones_like(ph)
    for got, name in zip(ora.find(ones, ph), ("craft_edges", "craft_dark", "craft_bright")):
        _hold("find " + name, got, planes[name], TOL, exact=True)
    e, p = planes["g2_dom_mag"], planes["g2_dom_phase"]
    for got, name in zip(ora.find(e, p), ("g2_find_edges", "g2_find_dark", "g2_find_bright")):
        _hold("find " + name, got, planes[name], _bound(e), exact=True)


@pytest.mark.parametrize("tag,cfg", [("g4", R.G4_DEFAULT), ("g4w4", R.G4_GENERIC)])
def test_oracle_g4_steer(ora, run, tag, cfg):
    planes, _ = run
    b = _stack(planes, tag + "_basis", 11)
    cases = [(F32(0.3), "g4_s0")] + ([(F32(-2.0), "g4_s1"), (planes["theta_map"], "g4_map")] if tag == "g4" else [])
    for theta, stem in cases:
        scalar = np.ndim(theta) == 0
        g, h = (ora.g4_steer_scalar if scalar else ora.g4_steer_map)(b, theta)
        wg, wh = A.g4_weights(theta)
        terms = _steer_terms(b, wg + wh)
        names = (stem + "_g", stem + "_h") if tag == "g4" else ("g4w4_g", "g4w4_h")
        _hold("%s %s g" % (tag, stem), g, planes[names[0]], _bound(*terms[:5]), exact=True)
        _hold("%s %s h" % (tag, stem), h, planes[names[1]], _bound(*terms[5:]), exact=True)


def test_oracle_generic_width_g2_steer(ora, run):
    planes, _ = run
    b = _stack(planes, "g2w3_basis", 7)
    g, h = ora.g2_steer_scalar(b, R.THETAS[0])
    terms = _steer_terms(b, _g2_weights(R.THETAS[0]))
    _hold("g2w3 steer g", g, planes["g2w3_g"], _bound(*terms[:3]), exact=True)
    _hold("g2w3 steer h", h, planes["g2w3_h"], _bound(*terms[3:]), exact=True)


# ---- the earlier known answers and float64 models, anchored on the run ----
@pytest.mark.parametrize("kind,stem", [(2, "g2_basis"), (4, "g4_basis")])
def test_known_answers_hold_the_fixture_basis(run, golden_dir, kind, stem):
    """the reference's tap tables (compiled in place, taps_ref.json) and kernel pairs, as known_answers restates sepFilter2D, on the
    fixture image: each plane to 1e-5 * max|plane|"""
    planes, _ = run
    want = _stack(planes, stem, 7 if kind == 2 else 11)
    got = K.basis_planes(golden_dir, kind, planes["image"])
    for p in range(len(want)):
        d, scale = float(np.abs(got[p].astype(F64) - want[p]).max()), float(np.abs(want[p]).max())
        print("known answers vs reference run, %s plane %d: %.3g of max|plane|" % (stem, p, d / scale))
        assert d <= 1e-5 * scale, (kind, p, d / scale)


def test_float64_models_hold_the_fixture(run):
    """orientation_model and angle_model (float64, no coefficient table) against what the reference's own code wrote, at the bounds
    they ask of the kernels"""
    planes, _ = run
    b = _stack(planes, "g2_basis", 7)
    want, bd = O.coefficients(b, 2), O.bound(b, 2)
    c = _coeffs(planes)
    rc = [float((np.abs(got.astype(F64) - w) / bd).max()) for got, w in zip(c, want)]
    s = O.strength(c[1], c[2])
    rs = float((np.abs(planes["g2_strength"] - s) / O.strength_bound(s)).max())
    dt = float(O.theta_error(planes["g2_theta"], O.theta(c[1], c[2], False)).max())
    print("f64 model vs reference run: C1..C3 %.3g %.3g %.3g of the bound, strength %.3g, theta %.3g rad" % (tuple(rc) + (rs, dt)))
    assert max(rc) <= 1.0 and rs <= 1.0 and dt <= O.THETA_TOL
    ph = planes["craft_phase"]
    worst = 0.0
    for k, (phi, signum) in enumerate(R.PHASE_WEIGHTS):
        worst = max(worst, float(np.abs(planes["craft_pw%d" % k] - A.phase_weights(ph, phi, signum)).max()))
    dfind = max(float(np.abs(planes[n] - w).max()) for n, w in zip(("craft_edges", "craft_dark", "craft_bright"), A.find_weights(ph)))
    print("f64 model vs reference run: phaseWeights %.3g, find on unit energy %.3g" % (worst, dfind))
    assert worst <= TOL and dfind <= TOL
    # ... and the steering polynomials, the energy and the magnitude / phase of the run's own planes
    for stem, theta, two in (("g2_s0", R.THETAS[0], None), ("g2_s1", R.THETAS[1], None), ("g2_s2", R.THETAS[2], None),
                             ("g2_map", planes["theta_map"], A.two_theta_f32(planes["theta_map"]))):
        g, h, e, m = A.g2_full(b, c, theta, two)
        r = max(float((np.abs(planes[stem + "_g5"] - g) / A.bound(b[:3], TOL)).max()), float((np.abs(planes[stem + "_h5"] - h) / A.bound(b[3:], TOL)).max()),
                float((np.abs(planes[stem + "_e"] - e) / A.bound(c, TOL)).max()))
        wg, wh = planes[stem + "_g5"], planes[stem + "_h5"]
        hyp = np.hypot(wg.astype(F64), wh.astype(F64))
        dm = float((np.abs(planes[stem + "_mag"] - hyp) / np.maximum(1.0, hyp)).max())
        dp = float(angle_diff(planes[stem + "_phase"], A.phase(wg, wh, False), 2 * np.pi).max())
        print("f64 model vs reference run, %s: g, h, e %.3g of the bound, magnitude %.3g, phase %.3g rad" % (stem, r, dm, dp))
        assert r <= 1.0 and dm <= TOL and dp <= 1e-5
    b4 = _stack(planes, "g4_basis", 11)
    for stem, theta in (("g4_s0", F32(0.3)), ("g4_s1", F32(-2.0)), ("g4_map", planes["theta_map"])):
        g, h = A.g4_steer(b4, theta)
        r = max(float((np.abs(planes[stem + "_g"] - g) / A.bound(b4[:5], TOL)).max()), float((np.abs(planes[stem + "_h"] - h) / A.bound(b4[5:], TOL)).max()))
        print("f64 model vs reference run, %s: g, h %.3g of the bound" % (stem, r))
        assert r <= 1.0


# ---- teeth: what a transcription slip would look like to these checks ----
def _excess(got, want, bound):
    return _dist(got, want) / bound


def test_teeth_h2b_h2c_swapped(ora, run):
    planes, _ = run
    b = _stack(planes, "g2_basis", 7)
    terms = _steer_terms(b, _g2_weights(R.THETAS[0]))
    bad = b[[0, 1, 2, 3, 5, 4, 6]]
    x = _excess(ora.g2_steer_scalar(bad, R.THETAS[0])[1], planes["g2_s0_h"], _bound(*terms[3:]))
    print("teeth: h2b / h2c swapped exceeds the steer bound %.3g x" % x)
    assert x >= TEETH
    # the pairing itself: a basis made with the two kernel pairs swapped
    assert _excess(ora.basis(2, planes["image"], 4, 0.67)[[0, 1, 2, 3, 5, 4, 6]], b, _bound(b)) >= TEETH


def test_teeth_h_bank_sign(ora, run):
    """a global sign of the H bank leaves C1..C3, the strength, theta and the magnitude alone; h and the phase see it"""
    planes, _ = run
    b = _stack(planes, "g2_basis", 7)
    terms = _steer_terms(b, _g2_weights(R.THETAS[0]))
    bad = b.copy()
    bad[3:] *= -1
    g, h, e, m, p = ora.g2_steer_scalar(bad, R.THETAS[0], _coeffs(planes))
    x = _excess(h, planes["g2_s0_h"], _bound(*terms[3:]))
    print("teeth: H bank negated exceeds the steer bound %.3g x" % x)
    assert x >= TEETH and _same(m, planes["g2_s0_mag"]) and all(_same(x_, y_) for x_, y_ in zip(ora.g2_orientation(bad), ora.g2_orientation(b)))
    strong = planes["g2_s0_mag"] > 1e-3 * planes["g2_s0_mag"].max()
    assert float(angle_diff(p, planes["g2_s0_phase"], 2 * np.pi)[strong].max()) >= TEETH * ANGLE_TOL
    # the basis planes themselves: all four H planes of the oracle negated
    ob = ora.basis(2, planes["image"], 4, 0.67)
    ob[3:] *= -1
    assert _excess(ob, b, _bound(b)) >= TEETH


def test_teeth_g4b_g4d_swapped(ora, run):
    planes, _ = run
    b = _stack(planes, "g4_basis", 11)
    wg, wh = A.g4_weights(F32(0.3))
    terms = _steer_terms(b, wg + wh)
    bad = b[[0, 3, 2, 1, 4, 5, 6, 7, 8, 9, 10]]
    x = _excess(ora.g4_steer_scalar(bad, F32(0.3))[0], planes["g4_s0_g"], _bound(*terms[:5]))
    print("teeth: g4b / g4d swapped exceeds the steer bound %.3g x" % x)
    assert x >= TEETH


def test_teeth_c3_coefficient(ora, run):
    planes, _ = run
    b = _stack(planes, "g2_basis", 7)
    b64 = b.astype(F64)
    c3 = ora.g2_orientation(b)[2]
    bad = (c3.astype(F64) + (1.6875 - 1.5) * b64[4] * b64[5]).astype(F32)      # C3 with 1.5 * h2b h2c in place of 1.6875 *
    x = _excess(bad, planes["g2_c3"], _bound(*[c * b64[i] * b64[j] for c, i, j in C_TERMS[3]]))
    print("teeth: C3's 1.6875 -> 1.5 exceeds the C3 bound %.3g x" % x)
    assert x >= TEETH


def test_teeth_phase_weights_gate(ora, run):
    """`> M_PI_2` read as `>=`: the two differ only where the folded error is exactly float(pi / 2) -- on the crafted plane the pixels
    +-float(pi / 2) for (0, signed), 0 and +-float(pi) for (pi / 2, unsigned), and float(pi / 2) for (pi, signed) -- and there by
    cos^2(float(pi / 2)) = 1.9e-15, nine orders below the stage bound of 1e-6: no distance can give this mutation teeth of 100 x.  What
    sees it is the bit pattern: the reference's own run left the nonzero value there, the mutant writes +0."""
    planes, _ = run
    ph = planes["craft_phase"]
    on_gate = F32(np.cos(F64(R.HALF_PI32))) ** 2
    assert 0 < on_gate < 1e-14
    hit = 0
    for k, (phi, signum) in enumerate(R.PHASE_WEIGHTS):
        p64, f = ph.astype(F64), float(phi)
        err = (np.abs(ph - phi) if signum else np.abs(np.abs(ph) - np.abs(phi))).astype(F32)
        err = np.minimum(err, (R.TWO_PI32 - err).astype(F32))
        at = err == R.HALF_PI32
        want = planes["craft_pw%d" % k]
        got = ora.phase_weights(ph, phi, signum)
        mutant = np.where(err >= R.HALF_PI32, F32(0), got)
        assert _same(got, want)
        if at.any():
            hit += int(at.sum())
            assert (want[at] == on_gate).all() and (_bits(want)[at] != 0).all()          # the reference's side of the gate
            assert not _same(mutant, want) and (_bits(mutant)[at] == 0).all()            # the mutant is on the other
            assert _dist(mutant, want) < TOL / TEETH                                     # ... and no distance bound would tell
        up = err == np.nextafter(R.HALF_PI32, F32(2))
        assert (_bits(want)[up] == 0).all()                                              # one float beyond the gate: closed
    print("teeth: the >= gate differs on %d crafted pixels, by %.3g each" % (hit, float(on_gate)))
    assert hit >= 5
