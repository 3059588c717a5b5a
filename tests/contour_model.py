"""numpy float32 models of contour thinning (cvs_nonmax, cvs_hysteresis) -- TEST INFRASTRUCTURE ONLY.

Every operation is in the order the contract of include/cvsteer_hip.h fixes; cos / sin come from the oracle's polar_to_cart (float of
a double cos / sin), which may differ from the kernel's ~1-ulp polynomial in the last bit: the tests allow for exactly that.  Linking
is scipy.ndimage.label with 8-connectivity, an algorithm independent of the kernels' propagation passes."""
import numpy as np
from scipy import ndimage

import oracle

F32 = np.float32


def directions(theta, sign_s=-1):
    """(c, s) of theta; sign_s = -1 is the contract's direction (c, -s) across the contour (+1 only to show that it would be wrong)"""
    c, s = oracle.polar_to_cart(np.ascontiguousarray(theta, dtype=F32))
    return c, (s if sign_s == -1 else -s)


def nonmax_parts(m, c, s):
    """one map: (output, backward sample, forward sample)"""
    m = np.ascontiguousarray(m, dtype=F32)
    rows, cols = m.shape
    p = np.pad(m, 1)   # neighbours outside the image read as 0.0f

    def at(dr, dc):
        return p[1 + dr:1 + dr + rows, 1 + dc:1 + dc + cols]

    with np.errstate(all="ignore"):
        ax, ay = np.abs(c), np.abs(s)
        major_x = ax >= ay
        w = np.where(major_x, ay / ax, ax / ay).astype(F32)
        om = (F32(1.0) - w).astype(F32)
        cpos, spos = c >= 0, s >= 0          # forward column step +1 / forward row step -1
        f_row = {dc: np.where(spos, at(-1, dc), at(1, dc)) for dc in (-1, 0, 1)}
        b_row = {dc: np.where(spos, at(1, dc), at(-1, dc)) for dc in (-1, 0, 1)}
        diag_f = np.where(cpos, f_row[1], f_row[-1])
        diag_b = np.where(cpos, b_row[-1], b_row[1])
        side_f = np.where(major_x, np.where(cpos, at(0, 1), at(0, -1)), f_row[0])
        side_b = np.where(major_x, np.where(cpos, at(0, -1), at(0, 1)), b_row[0])
        vf = ((om * side_f).astype(F32) + (w * diag_f).astype(F32)).astype(F32)
        vb = ((om * side_b).astype(F32) + (w * diag_b).astype(F32)).astype(F32)
        keep = (m > vb) & (m >= vf)
    return np.where(keep, m, F32(0.0)).astype(F32), vb, vf


def nonmax(maps, theta, sign_s=-1):
    """cvs_nonmax on a list of maps -> list of thinned maps"""
    c, s = directions(theta, sign_s)
    return [nonmax_parts(m, c, s)[0] for m in maps]


def hysteresis(v, low, high):
    """cvs_hysteresis on one plane -> uint8 0 / 255"""
    v = np.asarray(v, dtype=F32)
    with np.errstate(invalid="ignore"):
        strong = v > F32(high)
        cand = strong | ((v > F32(low)) & (v <= F32(high)))
    lab, _ = ndimage.label(cand, structure=np.ones((3, 3), bool))
    keep = np.isin(lab, np.unique(lab[strong])) & cand
    return np.where(keep, 255, 0).astype(np.uint8)


def decided(m, vb, vf):
    """pixels whose keep decision does not hinge on the last bits of cos / sin: both comparisons clear 1e-5 * max(|m|, |v|) and no
    neighbour is inf or NaN -- or m is +0.0 (which stores +0.0 kept or not)"""
    with np.errstate(all="ignore"):
        mb = np.abs(m - vb) > F32(1e-5) * np.maximum(np.abs(m), np.abs(vb))
        mf = np.abs(m - vf) > F32(1e-5) * np.maximum(np.abs(m), np.abs(vf))
    # a non-finite value in the 3 x 3 neighbourhood: which neighbours enter a sample with weight 0 hinges on the last bit of cos / sin
    # (|c| against |s| at +-pi/4), and 0 * inf is NaN
    p = np.pad(~np.isfinite(np.asarray(m, dtype=F32)), 1)
    rows, cols = np.shape(m)
    near = np.zeros((rows, cols), bool)
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            near |= p[1 + dr:1 + dr + rows, 1 + dc:1 + dc + cols]
    return ((mb & mf) & ~near) | (np.ascontiguousarray(m, dtype=F32).view(np.uint32) == 0)


# ---- geometry: steps and lines at 0, 22.5, .. 157.5 degrees ----
ANGLES = [22.5 * k for k in range(8)]


def feature_image(size, deg, kind, polarity, seed=0):
    """a step (kind 'step') or a thin line ('line') at `deg` degrees (x right, y down) a fraction of a pixel off the image centre, with a
    faint noise texture so that no two samples along the line are equal by symmetry; (image, signed distance to the line)"""
    y, x = np.mgrid[0:size, 0:size].astype(np.float64)
    a = np.deg2rad(deg)
    d = (x - size // 2 - 0.3) * -np.sin(a) + (y - size // 2 - 0.1) * np.cos(a)
    if kind == "step":
        img = 0.5 + polarity * 0.25 * np.tanh(d / 0.7)
    else:
        img = 0.5 + polarity * 0.4 * np.exp(-d * d / 4.5)
    img = img + 0.002 * np.random.default_rng(seed).random((size, size))
    return img.astype(F32), d


def geometry_report(raw, thin, d, deg, margin=12, frac=0.3, raw_frac=0.1):
    """checks of one thinned map: (kept off the line, bad cross-sections, thin un-thinned cross-sections, cross-sections looked at)"""
    size = raw.shape[0]
    thr = frac * float(np.nanmax(thin))
    kept = thin > thr
    band = np.abs(d) <= 3.0
    off = int(np.count_nonzero(kept & (np.abs(d) > 1.0)))
    a = np.deg2rad(deg)
    cols_major = abs(np.cos(a)) >= abs(np.sin(a))   # the line is closer to horizontal: cross-sections are columns
    bad = narrow = looked = 0
    for i in range(margin, size - margin):
        k = kept[:, i] if cols_major else kept[i, :]
        b = band[:, i] if cols_major else band[i, :]
        r = raw[:, i] if cols_major else raw[i, :]
        idx = np.nonzero(k & b)[0]
        pos = np.nonzero(b)[0]
        if pos.size == 0 or pos.min() < margin or pos.max() >= size - margin:
            continue
        looked += 1
        if not (len(idx) == 1 or (len(idx) == 2 and idx[1] - idx[0] == 1)):
            bad += 1
        if np.count_nonzero((r > raw_frac * float(np.nanmax(thin))) & b) < 3:
            narrow += 1
    return off, bad, narrow, looked
