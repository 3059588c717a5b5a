"""The per-pixel rules of the orientation peaks (cvs_orientation_peaks, include/cvsteer_hip.h, rules 3-9) in numpy -- TEST
INFRASTRUCTURE ONLY: neither product nor oracle code is imported here.

peaks_f32 applies the rules to sampled energies operation for operation in float32, so a kernel that keeps the contract equals it bit
for bit; peaks_f64 samples the energy with the float64 steering formulas of angle_model.py and applies the same rules in float64, and
says which pixels are `thin`: decided by a comparison whose two sides lie closer than float32 can be trusted to tell apart."""
import numpy as np

import angle_model as am

F32, F64 = np.float32, np.float64
PI_F = am.PI_F          # (float)pi as an exact value
THIN = 1e-5             # a comparison within this fraction of the pixel's largest sample is thin
THIN_CAP = 0.01         # a comparison of the two models is only made where at most this share of the pixels is thin
# float32 model against float64 model outside thin pixels, test_peaks_cpu.test_float32_model_against_float64 (64 x 96 smoothed noise, two
# seeds, both banks, K = 8, 16, 32, M = 4): worst angle difference 6.9e-5 rad (G4, K = 32), worst energy difference 6.0e-7 of the
# pixel's largest peak (G4, K = 32).  The tolerances are four times those.
F64_ANGLE_MEASURED, F64_ENERGY_MEASURED = 6.9e-5, 6.0e-7
F64_ANGLE_TOL, F64_ENERGY_TOL = 4 * F64_ANGLE_MEASURED, 4 * F64_ENERGY_MEASURED
# the worst angle error, in degrees, of the float32 model at the centre pixel of the 49 x 49 ridge image (ridge_image) over the
# directions 0, 20, 45, 77, 90 and 130 degrees, by (bank, K), measured on the CPU oracle's basis planes by
# test_peaks_cpu.test_one_ridge_peaks_across_its_direction; the tests hold a result to twice that.  Likewise either arm of the 20 / 110
# degree crossing, G4, K = 16.
RIDGE_MEASURED = {(2, 8): 0.5242, (2, 16): 0.0681, (2, 32): 0.0078, (4, 8): 1.1142, (4, 16): 0.1416, (4, 32): 0.0189}
RIDGE_BOUND = {k: 2.0 * v for k, v in RIDGE_MEASURED.items()}
CROSS_MEASURED = 0.1846
CROSS_BOUND = 2.0 * CROSS_MEASURED


def sample_angles(K):
    """theta_k = (float)((double)k * pi / K)"""
    return np.array([F32(F64(k) * np.pi / K) for k in range(K)], F32)


def step_f32(K):
    return F32(np.pi / K)


def _rules(e, M, min_energy, min_ratio, min_contrast, T, step, pi):
    """rules 3-9 on e[K, H, W] of type T; every constant is given in T.  -> angles[M], energies[M], count, and what the thin test needs"""
    K = e.shape[0]
    me, mr, mc = T(min_energy), T(min_ratio), T(min_contrast)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        finite = np.isfinite(e).all(axis=0)
        emax, emin = e.max(axis=0), e.min(axis=0)
        pixel = finite & ((emax - emin) > mc * emax)
        prev, nxt = np.roll(e, 1, axis=0), np.roll(e, -1, axis=0)
        local = (e > prev) & (e >= nxt)
        cand = local & (e > me) & (e >= mr * emax) & pixel[None]
        # e descending, ties by smaller k: a stable sort of the negated key keeps ascending k among equals
        key = np.where(cand, e, T(-np.inf))
        order = np.argsort(-key, axis=0, kind="stable")
        ncand = cand.sum(axis=0)
        count = np.minimum(ncand, M).astype(np.uint8)
        angles = np.full((M,) + e.shape[1:], T(-1.0), T)
        energies = np.zeros((M,) + e.shape[1:], T)
        for s in range(min(M, K)):
            k = order[s][None]
            p = np.take_along_axis(prev, k, axis=0)[0]
            c = np.take_along_axis(e, k, axis=0)[0]
            n = np.take_along_axis(nxt, k, axis=0)[0]
            num = p - n
            den = (p - T(2.0) * c) + n
            d = np.where(den < 0, (T(0.5) * num) / np.where(den < 0, den, T(1.0)), T(0.0)).astype(T)
            d = np.minimum(np.maximum(d, T(-0.5)), T(0.5))
            ang = (k[0].astype(T) + d) * step
            ang = np.where(ang < 0, ang + pi, ang)
            ang = np.where(~(ang < pi), ang - pi, ang)
            en = c - (T(0.25) * num) * d
            valid = s < ncand
            angles[s] = np.where(valid, ang, T(-1.0))
            energies[s] = np.where(valid, en, T(0.0))
    return angles, energies, count, (emax, emin, local, prev)


def peaks_f32(e, M, min_energy=0.0, min_ratio=0.0, min_contrast=0.0):
    """rules 3-9 on a [K, H, W] float32 array, every operation a float32 operation -> angles[M, H, W], energies[M, H, W] (float32),
    count[H, W] (uint8)"""
    e = np.ascontiguousarray(e, F32)
    assert e.ndim == 3 and e.dtype == F32
    a, en, c, _ = _rules(e, int(M), min_energy, min_ratio, min_contrast, F32, step_f32(e.shape[0]), F32(PI_F))
    assert a.dtype == F32 and en.dtype == F32
    return a, en, c


def energy_f64(basis, kind, K):
    """E(theta_k) = g^2 + h^2 in float64 from float32 basis planes, the sample angles taken as exact values -> [K, H, W]"""
    steer = am.g2_steer if kind == 2 else am.g4_steer
    out = []
    for th in sample_angles(K):
        g, h = steer(basis, float(th))
        out.append(g * g + h * h)
    return np.stack(out)


def peaks_f64(basis, kind, K, M, min_energy=0.0, min_ratio=0.0, min_contrast=0.0):
    """the same rules in float64 on energy_f64 -> angles, energies, count, thin[H, W].  The thresholds and the constants of rule 8 are
    the float32 values the call passes, taken as exact.  thin: some |e_k - e_(k+1)| < THIN * emax (the candidate rule and the order
    compare samples), or a threshold comparison of a local maximum, or the contrast comparison, lies within that band"""
    e = energy_f64(basis, kind, K)
    a, en, c, (emax, emin, local, prev) = _rules(e, int(M), float(F32(min_energy)), float(F32(min_ratio)), float(F32(min_contrast)), F64,
                                                 float(step_f32(K)), PI_F)
    with np.errstate(invalid="ignore"):
        band = THIN * emax
        thin = (np.abs(e - prev) < band[None]).any(axis=0)
        thin |= (local & (np.abs(e - float(F32(min_energy))) < band[None])).any(axis=0)
        thin |= (local & (np.abs(e - float(F32(min_ratio)) * emax[None]) < band[None])).any(axis=0)
        thin |= np.abs((emax - emin) - float(F32(min_contrast)) * emax) < band
        thin |= ~np.isfinite(e).all(axis=0)
    return a, en, c, thin


def match_sets(a32, e32, c32, a64, e64, c64):
    """peaks of two results as sets per pixel (equal counts assumed where compared): each peak of the first is matched to the nearest of
    the second by circular distance mod pi -> worst angle distance, worst |energy difference| / emax over the pixels with c32 == c64"""
    same = c32 == c64
    worst_a, worst_e = 0.0, 0.0
    M = a32.shape[0]
    scale = np.maximum(np.abs(e64).max(axis=0), 1e-300)
    for s in range(M):
        use = same & (s < c32)
        if not use.any():
            continue
        best_d = np.full(a32.shape[1:], np.inf)
        best_e = np.zeros(a32.shape[1:])
        for t in range(M):
            ok = use & (t < c64)
            d = am._f64(a32[s]) - am._f64(a64[t])
            d = np.abs(d) % np.pi
            d = np.minimum(d, np.pi - d)
            d = np.where(ok, d, np.inf)
            better = d < best_d
            best_d = np.where(better, d, best_d)
            best_e = np.where(better, np.abs(am._f64(e32[s]) - am._f64(e64[t])) / scale, best_e)
        worst_a = max(worst_a, float(best_d[use].max()))
        worst_e = max(worst_e, float(best_e[use].max()))
    return worst_a, worst_e


# ---- the inputs both test files use ----
def ridge_image(phis_deg, size=49, sigma=1.2, amplitude=255.0):
    """Gaussian ridges (sum) through the centre of a size x size image.  A ridge of direction phi runs along (cos phi, -sin phi) in
    (column, row) steps -- the row axis points down, as in cvs_nonmax's convention"""
    y, x = np.mgrid[0:size, 0:size].astype(F64)
    c = (size - 1) / 2.0
    img = np.zeros((size, size), F64)
    for phi in phis_deg:
        t = np.deg2rad(phi)
        dist = (x - c) * (-np.sin(t)) + (y - c) * (-np.cos(t))   # across the ridge: (cos, -sin)(phi + pi/2)
        img += amplitude * np.exp(-dist * dist / (2.0 * sigma * sigma))
    return img.astype(F32)


def smoothed_noise(rows, cols, seed, sigma=2.0):
    """white noise smoothed by a separable Gaussian (reflecting borders), float32"""
    rng = np.random.default_rng(seed)
    img = rng.standard_normal((rows, cols))
    r = int(np.ceil(4 * sigma))
    t = np.arange(-r, r + 1)
    k = np.exp(-t * t / (2.0 * sigma * sigma))
    k /= k.sum()
    pad = np.pad(img, r, mode="reflect")
    pad = np.apply_along_axis(lambda v: np.convolve(v, k, mode="valid"), 0, pad)
    pad = np.apply_along_axis(lambda v: np.convolve(v, k, mode="valid"), 1, pad)
    return (pad * 100.0).astype(F32)
