"""numpy / scipy model of cvs_link on one plane: hysteresis and prune as ONE labelling.  Independent of the device code and of the two
models it must agree with (contour_model.hysteresis followed by components_model.prune): the components of { v > low } are labelled once,
and a component is kept iff its largest value is > high and >= min_peak and it has >= min_area pixels."""
import numpy as np
from scipy import ndimage

F32 = np.float32


def link(v, low, high, min_area=0, min_peak=-np.inf):
    """-> (uint8 0 / 255, components kept)"""
    v = np.asarray(v, dtype=F32)
    with np.errstate(invalid="ignore"):
        w = v > F32(low)                                        # NaN is never in W
    lab, n = ndimage.label(w, structure=np.ones((3, 3), bool))
    if n == 0:
        return np.zeros(v.shape, np.uint8), 0
    idx = np.arange(1, n + 1)
    top = ndimage.maximum(np.where(w, v, F32(-np.inf)), lab, idx).astype(F32)
    area = np.bincount(lab.ravel(), minlength=n + 1)[1:]
    keep = (top > F32(high)) & (area >= int(min_area)) & (top >= F32(min_peak))
    lut = np.concatenate([[False], keep])
    return np.where(lut[lab], 255, 0).astype(np.uint8), int(np.count_nonzero(keep))


def case_grid(seed=0, shapes=((1, 1), (1, 37), (29, 1), (2, 2), (17, 31), (64, 96))):
    """the cases both test files walk: (name, plane, low, high, min_area, min_peak) -- random planes with NaN and negative pixels under
    every threshold family: low < high, low == high, a negative low, min_peak = -inf / between the thresholds / above high, min_area 0 / small / large"""
    rng = np.random.default_rng(seed)
    out = []
    for shape in shapes:
        for density in (0.15, 0.45, 0.8):
            v = (rng.random(shape) < density) * rng.random(shape, dtype=np.float32)
            v = v.astype(np.float32)
            k = max(1, v.size // 20)
            v.flat[rng.integers(0, v.size, k)] = np.nan
            v.flat[rng.integers(0, v.size, k)] = -rng.random(k, dtype=np.float32)
            v.flat[rng.integers(0, v.size, k)] = np.inf
            for low, high in ((0.2, 0.7), (0.5, 0.5), (-0.3, 0.4), (0.0, 0.0), (0.1, 2.0), (-1.0, -0.5)):
                for min_area, min_peak in ((0, -np.inf), (3, -np.inf), (0, 0.6), (5, 0.9), (1000, 0.0), (2, np.inf)):
                    out.append(("%dx%d d%.2f" % (shape[0], shape[1], density), v, low, high, min_area, min_peak))
    return out
