"""CPU tests of the 8-bit quantisation model (oracle/pyoracle.py: quantize_u8, convert_u8, normalize_u8) that every byte-writing
kernel is held against in tests/test_gpu_u8_reference.py.

The model is checked two ways: against the float64 ideal -- equal outside the tie band, within 1 inside it -- and against
plausible wrong quantisers (round half away, truncation, an FMA-contracted sum, f32 scale / shift, 255 * (1 / d)), each of
which must give other bytes on an input built here.  The planes built here (ties, separating inputs) feed the GPU tests too."""
import math
from fractions import Fraction

import numpy as np
import pytest

import oracle as ora

F32 = np.float32


# ----------------------------------------------------------------------------- the planes (shared with the GPU tests)
def random_plane(shape, seed):
    """wide-range signed values"""
    return (np.random.default_rng(seed).standard_normal(shape) * 37.0).astype(F32)


def offset_plane(shape, seed, lo=1000.0, span=3.0):
    """|lo| >> hi - lo: shift is large and cancels against v * scale"""
    return (lo + span * np.random.default_rng(seed).random(shape)).astype(F32)


def wide_plane(shape, seed):
    """magnitudes from 1 to 1e6, both signs"""
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(0, 6, shape)).astype(F32)


def nonfinite_plane(shape, seed):
    """a random plane with NaN, +inf, -inf and -0.0 sprinkled in (a normalise over it: range infinite, every byte 0)"""
    a = random_plane(shape, seed).ravel()
    rng = np.random.default_rng(seed + 1)
    idx = rng.permutation(a.size)
    k = max(1, a.size // 50)
    a[idx[:k]] = np.nan
    a[idx[k:2 * k]] = np.inf
    a[idx[2 * k:3 * k]] = -np.inf
    a[idx[3 * k:4 * k]] = -0.0
    return a.reshape(shape)


def nan_plane(shape, seed):
    """finite values with NaNs only: min / max skip them, the other pixels quantise as usual, NaN pixels give 0"""
    a = random_plane(shape, seed).ravel()
    a[np.random.default_rng(seed + 2).permutation(a.size)[:max(1, a.size // 20)]] = np.nan
    return a.reshape(shape)


def tie_planes():
    """exact .5 ties of the f32 op sequence -> [(plane, alpha, beta)]; alpha None = normalise.  Round half away, truncation and the
    ideal itself all disagree with half-to-even on them"""
    ints = np.arange(-4, 516, dtype=F32).reshape(10, 52)
    return [(ints, 0.5, 0.0),                                           # k / 2
            (np.arange(-3, 257, dtype=F32).reshape(4, 65), 1.0, 0.5),   # k + 1 / 2
            (np.arange(0, 511, dtype=F32).reshape(7, 73), None, 0.0)]   # lo = 0, hi = 510: scale = 0.5 exactly


def _fma_f32(v, s, t):
    """f32(v * s + t) with ONE rounding (what an FMA-contracted kernel computes)"""
    v = np.asarray(v, F32).astype(np.float64)
    p = v * float(s)                         # exact: 24 x 24 bits
    r = p + float(t)
    exact = (r - p) - float(t) == 0          # the double sum is exact, so one f64 -> f32 rounding is the FMA's
    out = r.astype(F32)
    for i in zip(*np.nonzero(~exact & np.isfinite(r))):
        out[i] = F32(float(Fraction(float(v[i])) * Fraction(float(s)) + Fraction(float(t))))
    return out


def _bytes(x):
    q = np.where(np.isnan(x), 0.0, np.clip(x, 0.0, 255.0))
    return q.astype(np.uint8)


# the wrong quantisers: each takes (plane, alpha, beta), alpha None = normalise
def _scale_shift(a, alpha, beta, recip=False, f32=False):
    if alpha is not None:
        return F32(alpha), F32(beta)
    lo, hi = ora.u8_minmax(a)
    if f32:
        d = F32(hi - lo)
        scale = F32(255.0) / d if d > 0 else F32(0.0)
        return F32(scale), F32(-lo * scale)
    d = float(hi) - float(lo)
    sd = 255.0 * (1.0 / d) if recip else 255.0 / d
    return F32(sd), F32(-float(lo) * sd)


def _x(a, scale, shift):
    with np.errstate(all="ignore"):
        return ((np.asarray(a, F32) * scale).astype(F32) + shift).astype(F32)


def variant_half_away(a, alpha, beta):
    x = _x(a, *_scale_shift(a, alpha, beta)).astype(np.float64)
    with np.errstate(all="ignore"):
        return _bytes(np.sign(x) * np.floor(np.abs(x) + 0.5))


def variant_truncate(a, alpha, beta):
    with np.errstate(all="ignore"):
        return _bytes(np.trunc(_x(a, *_scale_shift(a, alpha, beta)).astype(np.float64)))


def variant_fma(a, alpha, beta):
    return _bytes(np.rint(_fma_f32(a, *_scale_shift(a, alpha, beta)).astype(np.float64)))


def variant_f32_scale(a, alpha, beta):
    return _bytes(np.rint(_x(a, *_scale_shift(a, alpha, beta, f32=True)).astype(np.float64)))


def variant_recip(a, alpha, beta):
    return _bytes(np.rint(_x(a, *_scale_shift(a, alpha, beta, recip=True)).astype(np.float64)))


def model(a, alpha, beta):
    return ora.normalize_u8(a) if alpha is None else ora.convert_u8(a, alpha, beta)


def _near_ties(scale, shift, lo, hi, ulps=3):
    """f32 values v in [lo, hi] whose v * scale + shift lies next to a .5 tie: v = (k + 1/2 - shift) / scale and its neighbours"""
    t = np.arange(0, 256) + 0.5
    v = ((t - float(shift)) / float(scale)).astype(F32)
    out = [v]
    up = dn = v
    for _ in range(ulps):
        up = np.nextafter(up, F32(np.inf))
        dn = np.nextafter(dn, F32(-np.inf))
        out += [up, dn]
    v = np.concatenate(out)
    return v[(v >= lo) & (v <= hi)]


def separating_fma_planes():
    """small inputs on which an FMA-contracted sum gives other bytes than mul + add, found by a seeded search of random gains,
    offsets and ranges -> [(plane, alpha, beta)]: one convert (alpha, beta), one normalise (plane = lo, hi, then the pixels)"""
    rng = np.random.default_rng(2024)
    found = {}
    for _ in range(4000):
        if "convert" not in found:
            alpha, beta = F32(rng.uniform(0.1, 9.0)), F32(rng.uniform(-50.0, 50.0))
            v = _near_ties(alpha, beta, -1e4, 1e4)
            d = v[model(v, alpha, beta) != variant_fma(v, alpha, beta)]
            if d.size:
                found["convert"] = (np.resize(d[:8], (2, 4)).astype(F32), alpha, beta)
        if "normalize" not in found:
            lo = F32(rng.uniform(-100.0, 100.0))
            hi = F32(lo + rng.uniform(0.5, 300.0))
            v = _near_ties(*ora.u8_scale_shift(lo, hi), lo, hi)
            plane = np.concatenate([[lo, hi], v]).astype(F32)
            d = v[(model(plane, None, 0.0) != variant_fma(plane, None, 0.0))[2:]]
            if d.size:
                found["normalize"] = (np.resize(np.concatenate([[lo, hi], d[:6]]), (2, 4)).astype(F32), None, 0.0)
        if len(found) == 2:
            break
    assert len(found) == 2, "no separating input found"
    return [found["convert"], found["normalize"]]


def separating_recip_plane():
    """a small normalise input on which scale_d = 255 * (1 / d) gives other bytes than 255 / d -> (plane, None, 0).  The two forms
    differ by at most one float64 ulp, so they round to different f32 only where 255 / d lies within an ulp of an f32 midpoint:
    the seeded search picks such midpoints m, takes the float64 d next to 255 / m that an f32 pair makes exactly (hi - lo with
    hi = a 2^29 u, lo = b u), then pixels next to a tie"""
    rng = np.random.default_rng(77)
    for _ in range(20000):
        s = F32(rng.uniform(0.5, 500.0))
        d0 = 255.0 / ((float(s) + float(np.nextafter(s, F32(np.inf)))) / 2)
        e = math.frexp(d0)[1]
        n0 = round(math.ldexp(d0, 53 - e))
        for n in range(n0 - 4, n0 + 5):
            a = -(-n // 2 ** 29)
            b = a * 2 ** 29 - n
            if b >= 2 ** 24 or a >= 2 ** 24:
                continue
            hi, lo = F32(math.ldexp(a * 2 ** 29, e - 53)), F32(math.ldexp(b, e - 53))
            d = float(hi) - float(lo)
            if F32(255.0 / d) == F32(255.0 * (1.0 / d)) and F32(-float(lo) * (255.0 / d)) == F32(-float(lo) * (255.0 * (1.0 / d))):
                continue
            v = _near_ties(*ora.u8_scale_shift(lo, hi), lo, hi, ulps=2)
            plane = np.concatenate([[lo, hi], v]).astype(F32)
            diff = (model(plane, None, 0.0) != variant_recip(plane, None, 0.0))[2:]
            if diff.any():
                return np.resize(np.concatenate([[lo, hi], v[diff][:6]]), (2, 4)).astype(F32), None, 0.0
    raise AssertionError("no separating input found")


# ----------------------------------------------------------------------------- the model against the float64 ideal
@pytest.mark.parametrize("make,shape,seed", [(random_plane, (512, 1024), 1), (offset_plane, (512, 1024), 2),
                                             (wide_plane, (256, 512), 3), (nan_plane, (300, 301), 4)])
@pytest.mark.parametrize("mode", ["normalize", "convert", "convert_beta"])
def test_model_equals_the_ideal_outside_the_tie_band(make, shape, seed, mode):
    a = make(shape, seed)
    alpha, beta = {"normalize": (None, 0.0), "convert": (3.0, 0.0), "convert_beta": (0.37, 100.25)}[mode]
    if mode != "normalize" and make is offset_plane:
        alpha, beta = 85.0, -85000.0                     # the offset map through convertTo: same cancellation
    if mode != "normalize" and make is wide_plane:
        alpha = 1e-4 if mode == "convert" else 4e-5
    got = model(a, alpha, beta)
    off_band, in_band, band = ora.u8_against_ideal(got, a, alpha, beta)
    assert off_band == 0 and in_band == 0, (off_band, in_band)
    defined = np.isfinite(ora.u8_ideal(a, alpha, beta)).sum()
    assert defined > a.size // 2                                       # not vacuous: most pixels are held ...
    assert band <= 0.15 * defined, band                                # ... and the band is a small part of them
    ideal = ora.u8_ideal(a, alpha, beta)
    mid = np.isfinite(ideal) & (ideal > 0.5) & (ideal < 254.5)
    assert mid.sum() > 0.05 * a.size                                   # and not all saturated


def test_tie_band_is_where_the_model_leaves_the_ideal():
    """the model differs from clip(rint(ideal)) at a few pixels of a 2^20 plane, all inside the band (an exact check over
    the whole plane is needed to see them: a sampled or a +-1 check would not)"""
    a = random_plane((1024, 1024), 11)
    got = ora.normalize_u8(a)
    ideal = ora.u8_ideal(a)
    diff = got.astype(np.int32) != np.clip(np.rint(ideal), 0, 255)
    band = ora.u8_tie_band(a, ideal, *ora.u8_scale_shift(*ora.u8_minmax(a)))
    assert not (diff & ~band).any()
    assert band.sum() < 1e-3 * a.size


def test_exact_ties_round_half_to_even():
    (a, al, be), (b, bl, bb), (c, cl, cb) = tie_planes()
    ga = model(a, al, be)
    k = a.astype(np.int64)                                           # k / 2: k odd is a tie
    want = np.clip(np.where(k % 2 == 0, k // 2, np.where((k // 2) % 2 == 0, k // 2, k // 2 + 1)), 0, 255)
    assert np.array_equal(ga, want.astype(np.uint8))
    assert ga[np.where(a == 1)] == 0 and ga[np.where(a == 3)] == 2 and ga[np.where(a == 5)] == 2
    gb = model(b, bl, bb)                                            # k + 1/2 -> the even neighbour
    kb = b.astype(np.int64)
    assert np.array_equal(gb, np.clip(np.where(kb % 2 == 0, kb, kb + 1), 0, 255).astype(np.uint8))
    scale, shift = ora.u8_scale_shift(*ora.u8_minmax(c))
    assert scale == F32(0.5) and shift == 0
    gc = model(c, cl, cb)
    kc = c.astype(np.int64)
    assert np.array_equal(gc, np.where(kc % 2 == 0, kc // 2, np.where((kc // 2) % 2 == 0, kc // 2, kc // 2 + 1)).astype(np.uint8))
    assert gc.max() == 255 and gc[0, 1] == 0 and gc[0, 3] == 2


def test_saturation():
    a = np.array([[-1e30, -300.0, -0.51, -0.5, -0.49, 0.0, 254.49, 254.5, 255.49, 255.5, 256.0, 1e30]], F32)
    assert ora.convert_u8(a, 1.0).tolist() == [[0, 0, 0, 0, 0, 0, 254, 254, 255, 255, 255, 255]]
    b = np.array([[0.0, 1e-4, 5e-4, 6e-4, 0.1, 0.255, 0.256, 1.0, -0.1, 1e10]], F32)
    assert ora.convert_u8(b, 1000.0).tolist() == [[0, 0, 0, 1, 100, 255, 255, 255, 0, 255]]
    assert ora.convert_u8(b, 1000.0, -100.0).tolist() == [[0, 0, 0, 0, 0, 155, 156, 255, 0, 255]]


def test_nonfinite_and_degenerate_inputs():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    a = np.array([[nan, inf, -inf, -0.0, 0.0, 1.0, 2.0]], F32)
    assert ora.convert_u8(a, 100.0).tolist() == [[0, 255, 0, 0, 0, 100, 200]]
    assert ora.convert_u8(a, 0.0, 7.0).tolist() == [[0, 0, 0, 7, 7, 7, 7]]           # inf * 0 = NaN -> 0
    assert not ora.normalize_u8(a).any()                                             # range infinite: scale 0, shift NaN
    b = np.array([[nan, -0.0, 4.0, nan], [2.0, 0.0, nan, 1.0]], F32)                 # NaN skipped by min / max, NaN pixel -> 0
    assert ora.u8_minmax(b) == (0.0, 4.0)
    assert ora.normalize_u8(b).tolist() == [[0, 0, 255, 0], [128, 0, 0, 64]]
    assert ora.u8_minmax(np.full((3, 3), nan, F32)) == (inf, -inf)
    for plane in (np.full((3, 3), nan, F32), np.full((5, 4), 0.25, F32), np.full((1, 1), -7.0, F32), np.full((1, 1), nan, F32),
                  np.array([[inf, inf]], F32), np.array([[-inf, 3.0]], F32), np.array([[1.0, 1.0 + 1e-7 * 0]], F32)):
        assert not ora.normalize_u8(plane).any(), plane
    assert ora.convert_u8(np.full((1, 1), 2.5, F32), 1.0).tolist() == [[2]]
    assert ora.u8_scale_shift(1.0, 1.0) == (0.0, 0.0)
    s, t = ora.u8_scale_shift(-np.inf, 3.0)
    assert s == 0 and np.isnan(t)
    # hi - lo above DBL_EPSILON only in float64: a range of one ulp at 1.0 is not degenerate
    c = np.array([[1.0, np.nextafter(F32(1.0), F32(2.0))]], F32)
    assert ora.normalize_u8(c).tolist() == [[0, 255]]
    # the undefined pixels are skipped by the ideal check, not counted as agreeing
    assert np.isnan(ora.u8_ideal(a)).all() and np.isnan(ora.u8_ideal(a, 1.0)[0, :3]).all()


# ----------------------------------------------------------------------------- the model tells broken quantisers apart
VARIANTS = {"half_away": variant_half_away, "truncate": variant_truncate, "fma": variant_fma, "f32_scale_shift": variant_f32_scale,
            "recip_255_times_1_over_d": variant_recip}


def distinguishing_inputs():
    """every input the GPU tests use to separate the contract from its plausible variants"""
    return tie_planes() + separating_fma_planes() + [separating_recip_plane()] + [(offset_plane((37, 41), 5), None, 0.0)]


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_model_distinguishes_broken_quantisers(name):
    """in the style of test_golden_distinguishes_a_broken_oracle: each wrong quantiser gives other bytes than the model on at least
    one of the inputs the GPU tests feed the kernels"""
    bad = VARIANTS[name]
    hits = [i for i, (a, al, be) in enumerate(distinguishing_inputs()) if not np.array_equal(model(a, al, be), bad(a, al, be))]
    assert hits, name


def test_separating_inputs_are_small_and_stable():
    fma = separating_fma_planes()
    rec = separating_recip_plane()
    for a, al, be in fma + [rec]:
        assert a.shape == (2, 4) and a.dtype == F32 and np.isfinite(a).all()
    for a, al, be in fma:
        assert not np.array_equal(model(a, al, be), variant_fma(a, al, be))
    a, al, be = rec
    assert not np.array_equal(model(a, al, be), variant_recip(a, al, be))
    assert ora.u8_minmax(a) == (a[0, 0], a[0, 1])                   # normalise inputs carry their own lo and hi
    # the same search gives the same inputs every time (the GPU tests rebuild them)
    assert all(np.array_equal(x[0], y[0]) for x, y in zip(fma, separating_fma_planes()))


def test_normalize_minmax_u8_stays_the_float64_approximation():
    """the golden tests' normalize_minmax_u8 is the float64 form, kept as it was: within 1 of the model, not equal to it"""
    a = random_plane((1024, 1024), 11)
    d = np.abs(ora.normalize_minmax_u8(a).astype(np.int32) - ora.normalize_u8(a).astype(np.int32))
    assert d.max() == 1 and 0 < (d != 0).sum() < 100
