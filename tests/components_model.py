"""numpy / scipy models of the contour components (cvs_label, cvs_component_stats, cvs_contour_prune, cvs_contour_points) -- TEST
INFRASTRUCTURE ONLY.

Labelling is scipy.ndimage.label with 8-connectivity (a two-pass run-based algorithm on the CPU, nothing in common with the kernels'
union-find), renumbered here by the first raster occurrence of each component; statistics are plain numpy (bincount, minimum.at, a
lexicographic sort for the peak); prune and points follow from them."""
import numpy as np
from scipy import ndimage

COMPONENT_DTYPE = np.dtype([("area", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("first_x", "<i4"),
                            ("first_y", "<i4"), ("peak_x", "<i4"), ("peak_y", "<i4"), ("peak", "<f4")])
EIGHT = np.ones((3, 3), bool)


def foreground(mask):
    """f32: v > 0 (NaN, zeros, negatives are background); uint8: non-zero"""
    mask = np.asarray(mask)
    if mask.dtype == np.uint8:
        return mask != 0
    with np.errstate(invalid="ignore"):
        return np.asarray(mask, np.float32) > np.float32(0.0)


def label(mask):
    """-> (int32 labels, count): 0 = background, 1 .. count in raster order of each component's first pixel"""
    fg = foreground(mask)
    lab, n = ndimage.label(fg, structure=EIGHT)
    flat = lab.ravel()
    pos = np.flatnonzero(flat)
    vals, first = np.unique(flat[pos], return_index=True)      # first[i]: rank among the foreground pixels of vals[i]'s first pixel
    new = np.zeros(n + 1, np.int32)
    new[vals[np.argsort(first, kind="stable")]] = np.arange(1, n + 1, dtype=np.int32)
    return new[lab].astype(np.int32), int(n)


def stats(labels, count, weight=None):
    """cvs_component_stats: one record per label 1 .. count; pixels with other labels are skipped; a label nobody carries: area 0,
    positions -1, peak -inf"""
    labels = np.asarray(labels, np.int32)
    rows, cols = labels.shape
    t = np.zeros(count, COMPONENT_DTYPE)
    for f in ("x0", "y0", "x1", "y1", "first_x", "first_y", "peak_x", "peak_y"):
        t[f] = -1
    t["peak"] = -np.inf
    if count == 0:
        return t
    ok = (labels >= 1) & (labels <= count)
    ys, xs = np.nonzero(ok)
    k = labels[ok].astype(np.int64) - 1
    lin = ys.astype(np.int64) * cols + xs
    t["area"] = np.bincount(k, minlength=count)
    big = np.iinfo(np.int64).max
    x0, y0, first = np.full(count, big), np.full(count, big), np.full(count, big)
    x1, y1 = np.full(count, -1, np.int64), np.full(count, -1, np.int64)
    np.minimum.at(x0, k, xs)
    np.minimum.at(y0, k, ys)
    np.maximum.at(x1, k, xs)
    np.maximum.at(y1, k, ys)
    np.minimum.at(first, k, lin)
    seen = t["area"] > 0
    t["x0"][seen], t["y0"][seen], t["x1"][seen], t["y1"][seen] = x0[seen], y0[seen], x1[seen], y1[seen]
    t["first_x"][seen], t["first_y"][seen] = first[seen] % cols, first[seen] // cols
    if weight is not None:
        w = np.asarray(weight, np.float32)[ok]
        good = ~np.isnan(w)
        kk, ww, ll = k[good], w[good], lin[good]
        # per label: the largest weight first, +0.0 ahead of -0.0, then the smallest linear index
        order = np.lexsort((ll, np.signbit(ww), -ww.astype(np.float64), kk))
        kk, ww, ll = kk[order], ww[order], ll[order]
        head = np.ones(len(kk), bool)
        head[1:] = kk[1:] != kk[:-1]
        t["peak"][kk[head]] = ww[head]
        t["peak_x"][kk[head]] = ll[head] % cols
        t["peak_y"][kk[head]] = ll[head] // cols
    return t


def prune(mask, min_area, weight=None, min_peak=0.0):
    """cvs_contour_prune on one plane -> (uint8 0 / 255, components kept)"""
    lab, n = label(mask)
    t = stats(lab, n, weight)
    keep = t["area"] >= min_area
    if weight is not None:
        keep &= t["peak"] >= np.float32(min_peak)
    lut = np.concatenate([[False], keep])
    return np.where(lut[lab], 255, 0).astype(np.uint8), int(np.count_nonzero(keep))


def points(labels):
    """cvs_contour_points: (x, y, label) of every pixel with label != 0, in raster order"""
    labels = np.asarray(labels, np.int32)
    yx = np.argwhere(labels != 0)
    return np.stack([yx[:, 1], yx[:, 0], labels[labels != 0]], axis=1).astype(np.int32).reshape(-1, 3)
