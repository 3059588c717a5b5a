"""float64 statements of the per-pixel angle math, and the adversarial input families -- TEST INFRASTRUCTURE ONLY, numpy only.

Neither the product nor the oracle is imported here.  Every formula takes its float32 inputs as exact values and is evaluated in
float64; the only float32 step kept is one the reference makes on the INPUT of a formula and that decides whether the formula is
defined at all (the `theta * 2.0` plane of G2.cpp:175, see g2_full).  The families are pure functions of a seed, so a test without a
GPU and a test with one see the same arrays."""
import numpy as np

F32, F64 = np.float32, np.float64
ROWS, COLS = 131, 1021          # ragged: cols % 4 == 1, the dword tail of the per-pixel kernels; several workgroups
SIZE = ROWS * COLS

# the reference's float constants (SteerableFilters.cpp:49-50, G2.cpp:182,185 narrowed to f32 by the Mat1f expressions), as exact values
PI_F = float(F32(np.pi))
TWO_PI_F = float(F32(2 * np.pi))
HALF_PI_F = float(F32(np.pi / 2))
FLT_MAX = float(np.finfo(F32).max)


def _f64(a):
    return np.asarray(a, dtype=F64)


def _cs(theta):
    t = _f64(theta)
    with np.errstate(invalid="ignore"):
        return np.cos(t), np.sin(t)


# ---- steering ----
def g2_steer(b, theta):
    """G2.cpp:147-155: g = c^2 A - 2 c s B + s^2 C, h = c^3 HA - 3 c^2 s HB + 3 c s^2 HC - s^3 HD.  b: 7 planes -> g, h"""
    b = [_f64(x) for x in b]
    c, s = _cs(theta)
    g = c * c * b[0] - 2.0 * c * s * b[1] + s * s * b[2]
    h = c ** 3 * b[3] - 3.0 * c * c * s * b[4] + 3.0 * c * s * s * b[5] - s ** 3 * b[6]
    return g, h


def energy(c, theta, two_theta=None):
    """e = C1 + C2 cos 2 theta + C3 sin 2 theta (G2.cpp:163-164, 175-176).  two_theta=None takes 2 theta exactly (the scalar call: a
    double product, G2.cpp:163); a steer-by-map caller passes two_theta_f32(theta), the plane G2.cpp:175 hands to polarToCart"""
    t2 = 2.0 * _f64(theta) if two_theta is None else _f64(two_theta)
    c2, s2 = _cs(t2)
    return _f64(c[0]) + _f64(c[1]) * c2 + _f64(c[2]) * s2


def two_theta_f32(theta):
    """G2.cpp:175: `theta * 2.0` is a Mat1f -- a float32 plane.  The product is exact unless it overflows (|theta| > FLT_MAX / 2);
    there it is +-inf and the energy is undefined (NaN) exactly as at a non-finite theta"""
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(theta, F32) * F32(2.0)).astype(F64)


def g2_full(b, c, theta, two_theta=None):
    """-> g, h, e, magnitude"""
    g, h = g2_steer(b, theta)
    return g, h, energy(c, theta, two_theta), np.hypot(g, h)


def g4_weights(theta):
    """G4.cpp:99-112 / 116-119: c^4, -4 c^3 s, 6 c^2 s^2, -4 c s^3, s^4 and c^5, -5 c^4 s, 10 c^3 s^2, -10 c^2 s^3, 5 c s^4, -s^5"""
    c, s = _cs(theta)
    return ([c ** 4, -4.0 * c ** 3 * s, 6.0 * c * c * s * s, -4.0 * c * s ** 3, s ** 4],
            [c ** 5, -5.0 * c ** 4 * s, 10.0 * c ** 3 * s * s, -10.0 * c * c * s ** 3, 5.0 * c * s ** 4, -s ** 5])


def g4_steer(b, theta):
    """b: 11 planes (g4a..g4e, h4a..h4f) -> g, h"""
    b = [_f64(x) for x in b]
    wg, wh = g4_weights(theta)
    return sum(w * x for w, x in zip(wg, b[:5])), sum(w * x for w, x in zip(wh, b[5:]))


def bound(planes, tol=1e-6):
    """the stage tolerance scaled to the magnitudes that enter an output: tol * max(1, sum |plane_i|), per pixel"""
    return tol * np.maximum(1.0, sum(np.abs(_f64(p)) for p in planes))


# ---- arctangent ----
def wrap(a):
    """SteerableFilters::wrap: angles above float(pi) move down by float(2 pi)"""
    a = _f64(a)
    with np.errstate(invalid="ignore"):
        return np.where(a > PI_F, a - TWO_PI_F, a)


def fast_atan_0_2pi(y, x):
    """cv::cartToPolar's angle in the reference's OpenCV: the degree-7 odd polynomial in min / (max + DBL_EPSILON), degrees, then
    90 - a where |y| > |x|, 180 - a where x < 0, 360 - a where y < 0, then * pi / 180 -- all in float64.  Radians in [0, 2 pi]"""
    y, x = _f64(y), _f64(x)
    scale = float(F32(180.0 / np.pi))
    p1, p3, p5, p7 = (float(F32(F32(k) * F32(scale))) for k in
                      (0.9997878412794807, -0.3258083974640975, 0.1555786518463281, -0.04432655554792128))
    eps = float(F32(2.2204460492503131e-16))
    with np.errstate(all="ignore"):
        ax, ay = np.abs(x), np.abs(y)
        xge = ax >= ay
        mn, mx = np.where(xge, ay, ax), np.where(xge, ax, ay)
        c = mn / (mx + eps)
        c2 = c * c
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
        a = np.where(xge, a, 90.0 - a)
        a = np.where(x < 0, 180.0 - a, a)
        a = np.where(y < 0, 360.0 - a, a)
    return a * float(F32(np.pi / 180.0))


def atan_0_2pi(y, x):
    """np.arctan2 with negative results moved up by 2 pi"""
    with np.errstate(invalid="ignore"):
        a = np.arctan2(_f64(y), _f64(x))
        return np.where(a < 0, a + 2.0 * np.pi, a)


def phase(g, h, exact):
    """computeMagnitudeAndPhase's phase (G2.cpp:109-110): the angle of (g, h), wrapped"""
    return wrap(atan_0_2pi(h, g) if exact else fast_atan_0_2pi(h, g))


# ---- phaseWeights ----
def phase_weights(phase, phi, signum):
    """G2.cpp:179-186: err = |phase - phi| (signum) or ||phase| - |phi||; err = min(err, 2 pi - err); cos^2(err), 0 where
    |err| > pi / 2.  phi is the float32 the C ABI passes; 2 pi and pi / 2 are the reference's float32 constants"""
    p, phi = _f64(phase), float(F32(phi))
    with np.errstate(invalid="ignore"):
        err = np.abs(p - phi) if signum else np.abs(np.abs(p) - abs(phi))
        err = np.minimum(err, TWO_PI_F - err)
        lam = np.cos(err) ** 2
        return np.where(np.abs(err) > HALF_PI_F, 0.0, lam)


def find_weights(phase):
    """the weights of findEdges / findDarkLines / findBrightLines (G2.cpp:194-212)"""
    return (phase_weights(phase, HALF_PI_F, False), phase_weights(phase, 0.0, True), phase_weights(phase, PI_F, True))


# ---- input families ----
def _steps(v, n):
    """every float32 within n ulps of each v, v included"""
    v = np.asarray(v, F32).ravel()
    out = [v]
    for target in (F32(np.inf), F32(-np.inf)):
        w = v
        for _ in range(n):
            w = np.nextafter(w, target)
            out.append(w)
    return np.concatenate(out)


K_TWO_OVER_PI = F32(0.636619772)   # the reduction's multiplier (cvs_device_math.h, sincos_small)


def reduction_halfway_points():
    """the float32 x with |x| <= 8 at which float32(x * 2 / pi) is exactly n + 1/2 -- where the reduction's round-to-nearest-even is
    decided -- or, where no float32 hits it, the two that straddle it; each with its +-1 ulp neighbours"""
    out = []
    for n in range(-6, 6):
        x0 = F32((n + 0.5) * np.pi / 2)
        if abs(float(x0)) > 8.0:
            continue
        cand = _steps([x0], 16)
        prod = (cand * K_TWO_OVER_PI).astype(F32)
        hit = cand[prod == F32(n + 0.5)]
        if hit.size == 0:
            order = np.argsort(cand)
            cs, ps = cand[order], prod[order]
            i = int(np.searchsorted(ps, F32(n + 0.5)))
            hit = cs[max(i - 1, 0):i + 1]
        out.append(_steps(hit, 1))
        out.append(_steps([x0], 1))
    return np.concatenate(out)


LARGE = (10.0, 100.0, 1e4, 16777216.0, 1e10, 1e30, FLT_MAX)
TINY = (0.0, 1e-40, 1e-20)


def theta_special():
    """the hand-picked finite angles of theta_family(), 1-D float32 (duplicates kept: they cost nothing)"""
    quarter = np.array([F32(n * np.pi / 4) for n in range(-10, 11)], F32)   # |n pi / 4| <= 8
    eight = np.array([8.0, -8.0], F32)
    eights = np.concatenate([eight, np.nextafter(eight, F32(0)), np.nextafter(eight, np.array([np.inf, -np.inf], F32))])
    tiny = np.array([s * v for v in TINY for s in (1.0, -1.0)], F64).astype(F32)
    large = np.array([s * v for v in LARGE for s in (1.0, -1.0)], F64).astype(F32)
    return np.concatenate([_steps(quarter, 4), reduction_halfway_points(), eights, tiny, large])


NONFINITE_TAIL = np.array([np.nan, np.inf, -np.inf] * 4, F32)
N_SWEEP = 90001
N_DECADE = 300


def theta_family(seed=0):
    """(131, 1021) float32: a dense sweep of [-8, 8]; theta_special(); 300 random angles of either sign in each decade from 10 to
    1e8; a tail of NaN / +inf / -inf; padded with random angles in +-4 pi"""
    rng = np.random.default_rng(seed)
    parts = [np.linspace(-8.0, 8.0, N_SWEEP).astype(F32), theta_special()]
    for d in range(1, 8):
        mag = 10.0 ** (d + rng.random(N_DECADE))
        parts.append((mag * np.where(rng.random(N_DECADE) < 0.5, -1.0, 1.0)).astype(F32))
    parts.append(NONFINITE_TAIL)
    n = sum(p.size for p in parts)
    assert n < SIZE
    parts.append(((rng.random(SIZE - n) - 0.5) * 8.0 * np.pi).astype(F32))
    return np.concatenate(parts).reshape(ROWS, COLS)


def nms_thetas(seed=0):
    """the theta planes of the two thinning frames: the family, and the family turned by 180 degrees (every angle meets other pixels)"""
    th = theta_family(seed)
    return [th, np.ascontiguousarray(th[::-1, ::-1])]


NMS_SEEDS = (5, 6)   # the seeds of the thinning frames' maps (test_gpu_contours._random_case)


def bank_angles(n=100):
    """n scalar angles from theta_special(): every +-8 neighbour, tiny and large value, and an even pick of the rest"""
    sp = theta_special()
    n_fixed = 6 + 2 * len(TINY) + 2 * len(LARGE)
    fixed, rest = sp[-n_fixed:], sp[:-n_fixed]
    pick = rest[np.linspace(0, rest.size - 1, n - n_fixed).astype(int)]
    return np.concatenate([fixed, pick]).astype(F32)


GH_EXPONENTS = range(-40, 41)   # g^2 + h^2 stays a normal float32


def gh_family(seed=0):
    """(g, h, boundary): two (131, 1021) float32 planes and the mask of the pairs whose octant is decided by an exact comparison --
    the diagonals |g| == |h|, the axes with either sign of the zero, and (+-0, +-0).  The rest sweeps min / max over [0, 1] in
    every octant (which of |g|, |h| is larger, and both signs of each), at magnitudes 2^k, k = -40 .. 40"""
    g, h = [], []
    for sg in (0.0, -0.0):
        for sh in (0.0, -0.0):
            g.append(sg)
            h.append(sh)
    for k in GH_EXPONENTS:
        m = 2.0 ** k
        for a in (m, -m):
            for b in (m, -m):
                g.append(a)
                h.append(b)
            for z in (0.0, -0.0):
                g += [a, z]
                h += [z, a]
    nb = len(g)
    r = (SIZE - nb) // 8
    ratio = np.linspace(0.0, 1.0, r).astype(F32)
    mags = np.array([2.0 ** k for k in GH_EXPONENTS], F32)
    gs, hs = [np.array(g, F32)], [np.array(h, F32)]
    for o, (x_major, sx, sy) in enumerate((m, a, b) for m in (True, False) for a in (1, -1) for b in (1, -1)):
        mx = mags[(np.arange(r) + o) % mags.size]
        mn = (ratio * mx).astype(F32)           # a power of two: exact
        x, y = (mx, mn) if x_major else (mn, mx)
        gs.append((F32(sx) * x).astype(F32))
        hs.append((F32(sy) * y).astype(F32))
    pad = SIZE - nb - 8 * r
    rng = np.random.default_rng(seed)
    gs.append(rng.standard_normal(pad).astype(F32))
    hs.append(rng.standard_normal(pad).astype(F32))
    boundary = np.zeros(SIZE, bool)
    boundary[:nb] = True
    return (np.concatenate(gs).reshape(ROWS, COLS), np.concatenate(hs).reshape(ROWS, COLS), boundary.reshape(ROWS, COLS))


PHIS = (0.0, np.pi / 2, np.pi, 0.7, -2.0, 7.9, 8.1, 50.0)
