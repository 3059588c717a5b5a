"""numpy / Python model of the contour chains on the batch axis (cvs_contour_chains_batch) -- TEST ONLY, written from the contract in
include/cvsteer_hip.h: the per-plane model of chains_model.py concatenated, with global starts, the plane in the fourth column and the range
table.  `stacked` reads the same contract the other way round -- ONE run of the single-image model on the planes stacked with a blank row
between them, which is the contract's LIN order with a seam nothing can cross -- so the two can be held against each other."""
import numpy as np

import chains_model as CM


def chains_batch(masks):
    """(points (P, 2) int32 plane-local, chains (M, 4) int32 of (global start, length, flags, plane), ranges (n + 1, 2) int32)"""
    pts, tabs, ranges = [], [], []
    n_pts = n_chains = 0
    for z, mask in enumerate(masks):
        p, t = CM.chains(mask)
        t = t.copy()
        t[:, 0] += n_pts
        t[:, 3] = z
        ranges.append((n_chains, n_pts))
        pts.append(p)
        tabs.append(t)
        n_pts += len(p)
        n_chains += len(t)
    ranges.append((n_chains, n_pts))
    return (np.concatenate(pts).astype(np.int32).reshape(-1, 2), np.concatenate(tabs).astype(np.int32).reshape(-1, 4),
            np.array(ranges, np.int32).reshape(-1, 2))


def stacked(masks):
    """the same three arrays from one run of chains_model.chains on the planes stacked with one blank separator row between them"""
    masks = [np.asarray(m) for m in masks]
    rows, cols = masks[0].shape
    n = len(masks)
    tall = np.zeros((n * (rows + 1), cols), np.float32)
    for z, m in enumerate(masks):
        tall[z * (rows + 1):z * (rows + 1) + rows] = CM.foreground(m)
    pts, table = CM.chains(tall)
    plane = pts[:, 1] // (rows + 1)
    pts = np.stack([pts[:, 0], pts[:, 1] % (rows + 1)], axis=1).astype(np.int32).reshape(-1, 2)
    assert (pts[:, 1] < rows).all()
    table = table.copy()
    for c, (start, length, _, _) in enumerate(table.tolist()):
        assert (plane[start:start + length] == plane[start]).all()          # no chain crosses a seam
        table[c, 3] = plane[start]
    ranges = np.zeros((n + 1, 2), np.int32)
    for z in range(n + 1):
        ranges[z] = (int((table[:, 3] < z).sum()), int((plane < z).sum()))
    return pts, table, ranges
