"""float64 statement of the orientation stage (C1..C3, strength, theta), and its input families -- TEST INFRASTRUCTURE ONLY, numpy only.

Neither the product nor the oracle is imported here, and no coefficient table appears: C1..C3 are the Fourier projection of the
oriented energy E(theta) = g(theta)^2 + h(theta)^2 itself, with g and h steered in float64 (angle_model.g2_steer / g4_steer) from the
float32 basis planes taken as exact values.  E has even harmonics only, up to 6 (G2: g of degree 2, h of degree 3) and 10 (G4: degrees 4
and 5), so N_ANGLES = 16 samples over one period of pi project the mean and the second harmonic exactly (aliases fall on harmonic
2 + 32 m and 32 m - 2, far above 10).  The families are pure functions of their arguments, so a test without a GPU and a test with
one see the same arrays."""
import numpy as np

from angle_model import COLS, ROWS, atan_0_2pi, fast_atan_0_2pi, g2_steer, g4_steer, wrap
from helpers import rand_image, smooth_image

F32, F64 = np.float32, np.float64
N_ANGLES = 16
TOL = 1e-6              # the stage tolerance (tests/test_gpu_parity.py header)
THETA_TOL = 5e-6        # radians: half the project's angle tolerance of 1e-5, because theta is half an angle
N_G = {2: 3, 4: 5}      # G planes of a bank (the rest are the H planes)
WIDTH = {2: 4, 4: 6}    # the default tap half-widths
ZERO_BAND = 30          # rows at the bottom of an impulse family that no impulse reaches
EXPONENTS = 61          # impulse amplitudes 2^-30 .. 2^30: |C| from below 1e-27 to about 1e18 and no float32 square overflows (at +-60
                        # the float32 strength of the reference itself is inf)


def _f64(a):
    return np.asarray(a, dtype=F64)


# ---- the model ----
def coefficients(b, kind):
    """b: the 7 (kind 2) or 11 (kind 4) float32 basis planes -> C1, C2, C3 in float64: mean(E), 2 mean(E cos 2 theta),
    2 mean(E sin 2 theta) over theta_k = k pi / 16, k = 0 .. 15"""
    steer = g2_steer if kind == 2 else g4_steer
    c1 = c2 = c3 = 0.0
    for k in range(N_ANGLES):
        t = k * np.pi / N_ANGLES
        g, h = steer(b, t)
        e = g * g + h * h
        c1 = c1 + e
        c2 = c2 + e * np.cos(2.0 * t)
        c3 = c3 + e * np.sin(2.0 * t)
    return c1 / N_ANGLES, 2.0 * c2 / N_ANGLES, 2.0 * c3 / N_ANGLES


def bound(b, kind, tol=TOL):
    """the stage tolerance scaled to what enters a quadratic output: tol * max(1, (sum_G |b_i|)^2 + (sum_H |b_i|)^2), per pixel"""
    n = N_G[kind]
    sg = sum(np.abs(_f64(p)) for p in b[:n])
    sh = sum(np.abs(_f64(p)) for p in b[n:])
    return tol * np.maximum(1.0, sg * sg + sh * sh)


def strength(c2, c3):
    """|(C2, C3)| in float64; held to strength_bound()"""
    return np.hypot(_f64(c2), _f64(c3))


def strength_bound(s, tol=TOL):
    """tol * max(1, hypot): the absolute floor is there because the float32 squares underflow below about 1e-19, in the reference too"""
    return tol * np.maximum(1.0, _f64(s))


def theta(c2, c3, exact):
    """0.5 * wrap(angle of (C2, C3)), on the C2, C3 a launch itself stored (the decoupled-stage form: no strength mask is needed).
    Compare modulo pi (theta_error): the branch cut at angle == float(pi) may fall either way"""
    return 0.5 * wrap(atan_0_2pi(c3, c2) if exact else fast_atan_0_2pi(c3, c2))


def theta_error(got, want):
    """the distance of two orientations modulo pi -- or, where it is larger, how far `got` lies outside [-pi / 2, pi / 2]: modulo pi
    alone would not see a lost wrap, which moves theta by float(2 pi) / 2"""
    got = _f64(got)
    d = np.abs(got - _f64(want)) % np.pi
    return np.maximum(np.minimum(d, np.pi - d), np.maximum(np.abs(got) - np.pi / 2, 0.0))


# ---- input families ----
def _lattice(width, rows=ROWS, cols=COLS):
    step = 2 * width + 1
    h = step // 2
    return np.arange(h, rows - h - ZERO_BAND, step), np.arange(h, cols - h, step)


def impulse_family(width):
    """(131, 1021) float32 of zeros with isolated impulses, one per (2 width + 1)^2 cell so that no two supports overlap: each writes
    the outer product of the taps into the basis planes.  The n-th impulse in row-major order is s * 2^k, k = -30 + n % 61, s = -1
    where n // 61 is odd.  With power-of-two amplitudes the separable passes round identically in x and y, so C3 is exactly zero
    (with either sign) on the row and column through an impulse and C2 on its diagonals; the last ZERO_BAND rows (and two more) are
    a band where C1..C3 are all exactly zero"""
    img = np.zeros((ROWS, COLS), F32)
    ys, xs = _lattice(width)
    n = np.arange(ys.size * xs.size)
    amp = np.ldexp(np.where((n // EXPONENTS) % 2 == 1, -1.0, 1.0), -30 + n % EXPONENTS)
    img[np.ix_(ys, xs)] = amp.reshape(ys.size, xs.size).astype(F32)
    return img


MIXED_BLOCKS = (340, 680)


def mixed_family(seed=0):
    """(131, 1021) float32 in three column blocks: 0..339 smooth_image * 255 (byte-range values, a step edge), 340..679 uniform
    [0, 1), the rest standard normal * 2^k with k uniform in -12 .. 12 per pixel"""
    rng = np.random.default_rng(seed)
    a, b = MIXED_BLOCKS
    img = np.empty((ROWS, COLS), F32)
    img[:, :a] = smooth_image(ROWS, a) * F32(255.0)
    img[:, a:b] = rand_image(ROWS, b - a, seed=seed + 1)
    img[:, b:] = (rng.standard_normal((ROWS, COLS - b)) * np.ldexp(1.0, rng.integers(-12, 13, (ROWS, COLS - b)))).astype(F32)
    return img


U8_VALUES = (1, 2, 4, 8, 16, 32, 64, 128, 255)


def impulse_family_u8(width, seed=0):
    """(131, 1021) uint8: the impulse lattice with values cycling through 1, 2, 4, ..., 128, 255 on a zero plane, the right third
    (columns 680..) filled with random bytes"""
    img = np.zeros((ROWS, COLS), np.uint8)
    ys, xs = _lattice(width)
    n = np.arange(ys.size * xs.size)
    img[np.ix_(ys, xs)] = np.array(U8_VALUES, np.uint8)[n % len(U8_VALUES)].reshape(ys.size, xs.size)
    b = MIXED_BLOCKS[1]
    img[:, b:] = np.random.default_rng(seed).integers(0, 256, (ROWS, COLS - b), dtype=np.uint8)
    return img


def zero_band(width):
    """the rows below every impulse's support"""
    ys, _ = _lattice(width)
    return slice(int(ys[-1]) + width + 1, ROWS)


# ---- what a family must contain, counted on a launch's own C2, C3 ----
def axis_counts(c2, c3):
    """(pixels with C3 == 0 != C2, pixels with C2 == 0 != C3, exact (0, 0) pairs)"""
    c2, c3 = np.asarray(c2), np.asarray(c3)
    return (int(np.count_nonzero((c3 == 0) & (c2 != 0))), int(np.count_nonzero((c2 == 0) & (c3 != 0))),
            int(np.count_nonzero((c2 == 0) & (c3 == 0))))
