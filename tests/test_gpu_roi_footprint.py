"""GPU test (-m gpu): every caller-owned plane held to its ROI (tests/roi_guard.py) -- no byte outside a view is written.

include/cvsteer_hip.h, "Conventions": a call writes exactly rows x cols elements of each output plane and not one byte more, never writes
to an input, and what lies around an input view never changes a result.  An over-write by three columns, by one strip row or by a dense
copy where a pitched one was meant lands inside the caller's parent image: it faults nothing and changes no pixel of the view.

ONE TABLE (`row(entry point, case, body)`), one driver.  A body runs the call on the planes a context hands it; the context is either
DENSE -- planes of their own, the reference, on a fresh handle -- or GUARDED: every plane a view of a sentinel-filled parent, placed as the
test id says (roi_guard.PLACEMENTS).  The driver asserts, with no tolerance:
    1. the views equal the dense results bit for bit (which is also the read-footprint rule: the surroundings of every f32 input view
       hold NaN; byte inputs run twice, surroundings 0x00 and 0xFF);
    2. every output frame is intact;     3. every input parent is intact.
The dense call is the code the rest of the suite holds to the oracle and the models.  Every parent is allocated here and every call is a
legal call.  The table is generated from roi_guard.COVERED: a name in that list without a row fails at collection.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import cvsteer_amd as cv
import handle_sequences as H
import roi_guard as G
from cvsteer_amd import _lib as L
from cvsteer_amd import api
from cvsteer_amd.api import _plane as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, U8, S32 = np.float32, np.uint8, np.int32
BASIS, FULL = cv.SETUP_BASIS, cv.SETUP_FULL
LOW, HIGH = H.LOW, H.HIGH            # for maps that are uniform on [0, 1)
ANGLES = [0.3, -1.1, 2.0]
S1, S2 = (23, 67), (37, 260)
FALLBACK = {2: (12, 70), 4: (18, 70)}   # default taps on the two-pass fallback; cvs_pyr_down takes its stand-alone kernel
TINY = [(1, 1), (3, 5)]
DENSE_IN = "+dense-in"
OVERLAP_SHAPE = (1031, 1019)            # odd, and just past the 2^20-pixel switch to the overlapped host path
assert 1 << 20 <= OVERLAP_SHAPE[0] * OVERLAP_SHAPE[1] < (1 << 20) * 1.01


def close(f):
    f.__del__()


def img(shape, seed, u8=False):
    return H.make_image((shape[0], shape[1], seed, u8))


def ready(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def prep(f, shape, flags=FULL, seed=50):
    """image size and state from a dense device image: not part of the call under test"""
    f.setup(ready(img(shape, seed)), flags)


def raw(f, name, *args):
    rc = getattr(L.lib(), name)(f._h, *args)
    if rc:
        raise cv.CvsError(rc, name, L.lib().cvs_last_error(f._h).decode())


def ptr(a):
    if a is None or (a.numel() if torch.is_tensor(a) else a.size) == 0:
        return None
    return C.c_void_p(a.data_ptr() if torch.is_tensor(a) else a.ctypes.data)


def half(shape):
    return ((shape[0] + 1) // 2, (shape[1] + 1) // 2)


def mask03(shape, seed=5):
    """one random mask of density 0.3"""
    return ((np.random.default_rng(seed).random(shape) < 0.3) * 255).astype(U8)


class Ctx:
    """hands a body its planes: dense (placement None) or guarded views; remembers the parents for the checks"""

    def __init__(self, shape, mem, make, placement=None, surround=None):
        self.shape, self.mem, self.make, self.placement, self.surround = tuple(shape), mem, make, placement, surround
        self.dev = DEV if mem == "dev" else None
        self.memflag = L.MEM_DEVICE if mem == "dev" else L.MEM_HOST
        self.frames, self.inputs, self.handles = [], [], []
        self.in_placement = placement
        if placement is not None and placement.endswith(DENSE_IN):   # guarded outputs, dense inputs (still held to their bits)
            self.placement, self.in_placement = placement[:-len(DENSE_IN)], "dense"

    def _dense(self, values):
        a = np.ascontiguousarray(values).copy()
        return torch.from_numpy(a).to(DEV) if self.dev else a

    def _fresh(self, shape, dtype):
        return G.Parent(shape, dtype, self.dev).buf     # dense, and sentinel-filled like the views' parents

    def inp(self, values, haxis=None):
        if self.placement is None:
            return self._dense(values)
        p, v = G.guard_input(values, self.in_placement, self.dev, self.surround if values.dtype == U8 else None, haxis)
        self.inputs.append(p)
        return v

    def inp_array(self, values):
        if self.placement is None:
            return self._dense(values)
        p, v = G.guard_input_array(values, *((0, 0) if self.in_placement == "dense" else (8, 16)), self.dev)
        self.inputs.append(p)
        return v

    def outs(self, specs):
        if self.placement is None:
            return [self._fresh(s, d) for s, d in specs]
        parents, views = G.windows(specs, self.placement, self.dev)
        self.frames += parents
        return views

    def out(self, shape, dtype=F32):
        return self.outs([(shape, dtype)])[0]

    def block(self, shape, haxis, dtype=F32):
        if self.placement is None:
            return self._fresh(shape, dtype)
        p, inner = G.block(shape, haxis, self.placement, dtype, self.dev)
        self.frames.append(p)
        return inner

    def inout(self, values):
        """a plane the call reads and writes in place: values inside, the output sentinel around"""
        if self.placement is None:
            return self._dense(values)
        p, v = G.window(values.shape, values.dtype, self.placement, self.dev)
        if self.dev:
            v.copy_(torch.from_numpy(np.ascontiguousarray(values)))
        else:
            v[...] = values
        self.frames.append(p)
        return v

    def array(self, n, dtype):
        """an output array: 8 elements guarded in front of it, 16 behind it"""
        if self.placement is None:
            return self._fresh(tuple(n) if isinstance(n, (tuple, list)) else (n,), dtype)
        p, v = G.array(n, dtype, 8, 16, self.dev)
        self.frames.append(p)
        return v


class Row:
    def __init__(self, entry, case, fn, kind=2, taps=None, tags=(), bytes_in=False, bytes_any=False, lists=False, host=True):
        self.entry, self.case, self.fn, self.kind, self.taps, self.tags = entry, case, fn, kind, taps, tuple(tags)
        self.bytes_in, self.bytes_any, self.lists, self.host = bytes_in, bytes_any or bytes_in, lists, host
        self.id = "%s:%s" % (entry[4:], case)

    def make(self):
        if self.taps:
            return cv.SteerableFiltersG2(None, self.taps[1], self.taps[2])
        return cv.SteerableFiltersG2(None) if self.kind == 2 else cv.SteerableFiltersG4(None, extensions=True)


ROWS = []


def row(entry, case, fn, **kw):
    ROWS.append(Row(entry, case, fn, **kw))


# ================================================================ the table
# ---------------------------------------------------------------- filter bank: cvs_setup_steer, cvs_pipeline, cvs_pipeline_batch, pyramid
def b_setup_steer(flags):
    def fn(c, f):
        x = c.inp(img(c.shape, 1))
        g, h = c.outs([(c.shape, F32)] * 2)
        f.setup_steer(x, 0.7, flags, out=(g, h))
        return [g, h]
    return fn


row("cvs_setup_steer", "g2-basis", b_setup_steer(BASIS), tags=("strip",))
row("cvs_setup_steer", "g2-full", b_setup_steer(FULL), tags=("strip", "overlap"))
row("cvs_setup_steer", "g4-basis", b_setup_steer(BASIS), kind=4, tags=("strip",))
row("cvs_setup_steer", "g4-full", b_setup_steer(FULL), kind=4, tags=("strip",))
row("cvs_setup_steer", "w6-full", b_setup_steer(FULL), taps=(2, 6, 0.5))


def b_pipeline(sel, dtype=F32, gain=None, persist=True):
    def fn(c, f):
        if not persist:
            f.set_persist(False)
        if gain is not None:
            f.set_u8_gain(gain)
        x = c.inp(img(c.shape, 2))
        views = c.outs([(c.shape, dtype)] * len(sel))
        outs = [None] * 8
        for k, v in zip(sel, views):
            outs[k] = v
        f.pipeline(x, out=outs)
        return views
    return fn


ALL8, FEAT3 = tuple(range(8)), (5, 6, 7)
row("cvs_pipeline", "g2-all8", b_pipeline(ALL8), tags=("strip", "overlap"))
row("cvs_pipeline", "g2-feat3", b_pipeline(FEAT3), tags=("strip",))
row("cvs_pipeline", "g2-feat3-u8-gain", b_pipeline(FEAT3, U8, gain=40.0, persist=False), tags=("strip",), bytes_any=True)
row("cvs_pipeline", "g2-feat3-u8-norm", b_pipeline(FEAT3, U8, gain=0.0, persist=False), tags=("strip", "overlap"), bytes_any=True)
row("cvs_pipeline", "g2-all8-stateless", b_pipeline(ALL8, persist=False), tags=("strip",))
row("cvs_pipeline", "g4-all8", b_pipeline(ALL8), kind=4, tags=("strip",))
row("cvs_pipeline", "g4-feat3-u8", b_pipeline(FEAT3, U8), kind=4, tags=("strip",), bytes_any=True)
row("cvs_pipeline", "w6-all8", b_pipeline(ALL8), taps=(2, 6, 0.5))


def b_batch_block(sel, u8_in, persist):
    """the regular block form: [3][H][W] frames in, `out` a column slice of a wider 4-D tensor"""
    def fn(c, f):
        if not persist:
            f.set_persist(False)
        x = c.inp(np.stack([img(c.shape, 10 + i, u8_in) for i in range(3)]), 1)
        out = c.block((3, len(sel)) + c.shape, 2)
        f.pipeline_batch(x, out=out, outputs=sel)
        return [out]
    return fn


def b_batch_table(sel, u8_in, persist):
    """the frame-table form: every frame and every output a plane of its own"""
    def fn(c, f):
        if not persist:
            f.set_persist(False)
        xs = [c.inp(img(c.shape, 10 + i, u8_in)) for i in range(3)]
        views = c.outs([(c.shape, F32)] * (3 * len(sel)))
        f.pipeline_batch(xs, out=[views[i * len(sel):(i + 1) * len(sel)] for i in range(3)], outputs=sel)
        return views
    return fn


row("cvs_pipeline_batch", "block-f32-state", b_batch_block(ALL8, False, True), tags=("strip",))
row("cvs_pipeline_batch", "block-u8-outputs-only", b_batch_block(FEAT3, True, False), tags=("strip",), bytes_in=True)
row("cvs_pipeline_batch", "table-f32-outputs-only", b_batch_table(FEAT3, False, False), tags=("strip",))
row("cvs_pipeline_batch", "table-u8-state", b_batch_table((0, 1, 4, 7), True, True), tags=("strip",), bytes_in=True)


def b_setup_pyr(c, f):
    x = c.inp(img(c.shape, 3))
    nxt = c.out(half(c.shape))
    f.setup_pyr(x, FULL if f.KIND == 2 else BASIS, out=nxt)
    return [nxt]


def b_pyr_down(c, f):
    x, dst = c.inp(img(c.shape, 3)), c.out(half(c.shape))
    f._bind_stream(x, dst)
    ps, pd = P(x), P(dst)
    raw(f, "cvs_pyr_down", C.byref(ps), C.byref(pd))
    return [dst]


def b_pyramid_setup(c, f):
    hs = [f] + [c.make() for _ in range(2)]
    c.handles += hs[1:]
    x = c.inp(img(c.shape, 3))
    s1 = half(c.shape)
    levels = c.outs([(s1, F32), (half(s1), F32)])
    api.pyramid_setup(hs, x, levels, FULL if f.KIND == 2 else BASIS)
    return levels + [hs[2].basis(0)]


row("cvs_setup_pyr", "g2-full", b_setup_pyr, tags=("strip",))
row("cvs_setup_pyr", "g4-basis", b_setup_pyr, kind=4, tags=("strip",))
row("cvs_setup_pyr", "w6-full", b_setup_pyr, taps=(2, 6, 0.5))
row("cvs_pyr_down", "f32", b_pyr_down, tags=("point",))     # (no basis launch: cvs_launch_info says nothing about it)
row("cvs_pyramid_setup", "g2-3-levels", b_pyramid_setup, tags=("strip",))


# ---------------------------------------------------------------- state read-out and the per-pixel entries
def b_read_state(c, f):
    prep(f, c.shape)
    views = c.outs([(c.shape, F32)] * 4)
    for code, v in zip((L.PLANE_BASIS0 + 1, L.PLANE_C2, L.PLANE_THETA, L.PLANE_STRENGTH), views):
        f._bind_stream(v)
        p = P(v)
        raw(f, "cvs_read_state", code, C.byref(p))
    return views


row("cvs_read_state", "basis-c2-theta-strength", b_read_state)


def b_steer_scalar(n):
    def fn(c, f):
        prep(f, c.shape)
        views = c.outs([(c.shape, F32)] * n)
        f.steer(0.3, full=(n == 5), out=views)
        return views
    return fn


def b_steer_map(n, own_theta):
    def fn(c, f):
        prep(f, c.shape)
        th = None if own_theta else c.inp(H.make_theta(c.shape, 3))
        views = c.outs([(c.shape, F32)] * n)
        f.steer(th, full=(n == 5), out=views)
        return views
    return fn


row("cvs_steer_scalar", "g2-full5", b_steer_scalar(5), tags=("point",))
row("cvs_steer_scalar", "g4-gh", b_steer_scalar(2), kind=4, tags=("point",))
row("cvs_steer_map", "g2-gh-own-theta", b_steer_map(2, True), tags=("point",))
row("cvs_steer_map", "g2-full5", b_steer_map(5, False), tags=("point",))
row("cvs_steer_map", "g4-full5", b_steer_map(5, False), kind=4, tags=("point",))


def b_bank_views(c, f):
    prep(f, c.shape)
    views = c.outs([(c.shape, F32)] * 6)
    f.steer_bank(ANGLES, out=[views[:3], views[3:]])
    return views


def b_bank_hkw(c, f):
    """rows interleaved [H][K][W], W a column slice"""
    prep(f, c.shape)
    blocks = [c.block((c.shape[0], 3, c.shape[1]), 0) for _ in range(2)]
    f.steer_bank(ANGLES, out=[b.permute(1, 0, 2) if torch.is_tensor(b) else b.transpose(1, 0, 2) for b in blocks])
    return blocks


def b_bank_k33(c, f):
    """K = KMAX + 1: two launches over a [K][H][W] block"""
    prep(f, c.shape)
    blocks = [c.block((33,) + c.shape, 1) for _ in range(2)]
    f.steer_bank(np.linspace(-3.0, 3.0, 33), out=blocks)
    return blocks


row("cvs_steer_bank", "views", b_bank_views, tags=("point",))
row("cvs_steer_bank", "hkw-block", b_bank_hkw, tags=("point",))
row("cvs_steer_bank", "k33-block", b_bank_k33, tags=("point",))


def b_mag_phase(c, f):
    prep(f, c.shape, BASIS)
    g, h = c.inp(H.make_map(c.shape, 1) - np.float32(0.5)), c.inp(H.make_map(c.shape, 2) - np.float32(0.5))
    mag, ph = c.outs([(c.shape, F32)] * 2)
    f._bind_stream(g, h, mag, ph)
    pg, ph_, pm, pp = P(g), P(h), P(mag), P(ph)
    raw(f, "cvs_mag_phase", C.byref(pg), C.byref(ph_), C.byref(pm), C.byref(pp))
    return [mag, ph]


def b_wrap(in_place):
    def fn(c, f):
        prep(f, c.shape, BASIS)
        vals = H.make_map(c.shape, 3) * np.float32(9.0)
        a = c.inout(vals) if in_place else c.inp(vals)
        o = a if in_place else c.out(c.shape)
        f._bind_stream(a, o)
        pa, po = P(a), P(o)
        raw(f, "cvs_wrap", C.byref(pa), C.byref(po))
        return [o]
    return fn


def b_phase_weights(c, f):
    prep(f, c.shape, BASIS)
    ph, lam = c.inp(H.make_theta(c.shape, 4) * np.float32(2.0)), c.out(c.shape)
    f._bind_stream(ph, lam)
    pp, pl = P(ph), P(lam)
    raw(f, "cvs_phase_weights", C.byref(pp), C.byref(pl), 0.5, 1, 2.0)
    return [lam]


def b_find(which):
    def fn(c, f):
        prep(f, c.shape, BASIS)
        e, ph = c.inp(H.make_map(c.shape, 5)), c.inp(H.make_theta(c.shape, 6) * np.float32(2.0))
        views = c.outs([(c.shape, F32)] * sum(which))
        it = iter(views)
        planes = [P(next(it)) if w else None for w in which]
        f._bind_stream(e, ph, *views)
        pe, pp = P(e), P(ph)
        raw(f, "cvs_find", C.byref(pe), C.byref(pp), *[C.byref(p) if p is not None else None for p in planes])
        return views
    return fn


row("cvs_mag_phase", "f32", b_mag_phase, tags=("point",))
row("cvs_wrap", "out-of-place", b_wrap(False), tags=("point",))
row("cvs_wrap", "in-place", b_wrap(True), tags=("point",))
row("cvs_phase_weights", "f32", b_phase_weights, tags=("point",))
row("cvs_find", "all-three", b_find((True, True, True)), tags=("point",))
row("cvs_find", "dark-alone", b_find((False, True, False)), tags=("point",))


def b_peaks(as_block):
    def fn(c, f):
        prep(f, c.shape, BASIS)
        if as_block:
            blk = c.block((2, 2) + c.shape, 2)
            ang, en, cnt = blk[0], blk[1], c.out(c.shape, U8)
            res = [blk, cnt]
        else:
            views = c.outs([(c.shape, F32)] * 4 + [(c.shape, U8)])
            ang, en, cnt = views[:2], views[2:4], views[4]
            res = views
        f.orientation_peaks(8, 2, out=(ang, en, cnt))
        return res
    return fn


row("cvs_orientation_peaks", "g2-views", b_peaks(False), tags=("point",), bytes_any=True)
row("cvs_orientation_peaks", "g4-block", b_peaks(True), kind=4, tags=("point",), bytes_any=True)


# ---------------------------------------------------------------- contour thinning, linking, components
def b_nonmax(own_theta):
    def fn(c, f):
        prep(f, c.shape)
        maps = [c.inp(H.make_map(c.shape, 10 + k)) for k in range(3)]
        th = None if own_theta else c.inp(H.make_theta(c.shape, 7))
        outs = c.outs([(c.shape, F32)] * 3)
        f.nonmax(maps, theta=th, out=outs)
        return outs
    return fn


def b_nonmax_batch(as_block):
    def fn(c, f):
        prep(f, c.shape)
        vals = np.stack([np.stack([H.make_map(c.shape, 20 + 2 * i + k) for k in range(2)]) for i in range(2)])
        ths = np.stack([H.make_theta(c.shape, 30 + i) for i in range(2)])
        if as_block:
            x, th, out = c.inp(vals, 2), c.inp(ths, 1), c.block(vals.shape, 2)
            f.nonmax_batch(x, theta=th, out=out)
            return [out]
        xs = [[c.inp(vals[i, k]) for k in range(2)] for i in range(2)]
        th = [c.inp(ths[i]) for i in range(2)]
        views = c.outs([(c.shape, F32)] * 4)
        f.nonmax_batch(xs, theta=th, out=[views[:2], views[2:]])
        return views
    return fn


row("cvs_nonmax", "three-maps", b_nonmax(False), tags=("point",))
row("cvs_nonmax", "own-theta", b_nonmax(True), tags=("point",))
row("cvs_nonmax_batch", "table", b_nonmax_batch(False), tags=("point",))
row("cvs_nonmax_batch", "block", b_nonmax_batch(True), tags=("point",))


def b_hysteresis(dtype):
    def fn(c, f):
        prep(f, c.shape, BASIS)
        maps = [c.inp(H.make_map(c.shape, 40 + k)) for k in range(2)]
        outs = c.outs([(c.shape, dtype)] * 2)
        f.hysteresis(maps, LOW, HIGH, out=outs)
        return outs
    return fn


def b_label(u8_mask):
    def fn(c, f):
        prep(f, c.shape, BASIS)
        m = mask03(c.shape) if u8_mask else np.where(H.make_map(c.shape, 41) > 0.6, H.make_map(c.shape, 41), np.float32(0)).astype(F32)
        mv, lab = c.inp(m), c.out(c.shape, S32)
        _, count = f.label(mv, out=lab)
        return [lab, np.array([count], S32)]
    return fn


def b_prune(dtype):
    def fn(c, f):
        prep(f, c.shape, BASIS)
        masks = [c.inp(mask03(c.shape, 42 + k)) for k in range(2)]
        ws = [c.inp(H.make_map(c.shape, 44 + k)) for k in range(2)]
        outs = c.outs([(c.shape, dtype)] * 2)
        _, kept = f.prune(masks, 2, weight=ws, min_peak=0.5, out=outs, return_kept=True)
        return outs + [np.array(kept, S32)]
    return fn


def b_link(dtype, as_block):
    def fn(c, f):
        prep(f, c.shape, BASIS)
        vals = np.stack([H.make_map(c.shape, 46 + k) for k in range(3)])
        if as_block:
            x, out = c.inp(vals, 1), c.block(vals.shape, 1, dtype)
            f.link(x, LOW, HIGH, min_area=2, min_peak=0.85, out=out)
            return [out]
        xs = [c.inp(v) for v in vals]
        outs = c.outs([(c.shape, dtype)] * 3)
        f.link(xs, LOW, HIGH, min_area=2, min_peak=0.85, out=outs)
        return outs
    return fn


row("cvs_hysteresis", "u8-out", b_hysteresis(U8), bytes_any=True)
row("cvs_hysteresis", "f32-out", b_hysteresis(F32))
row("cvs_label", "f32-mask", b_label(False))
row("cvs_label", "u8-mask", b_label(True), bytes_in=True)
row("cvs_contour_prune", "u8-out", b_prune(U8), bytes_in=True)
row("cvs_contour_prune", "f32-out", b_prune(F32), bytes_in=True)
row("cvs_link", "table-u8", b_link(U8, False), bytes_any=True)
row("cvs_link", "table-f32", b_link(F32, False))
row("cvs_link", "block-u8", b_link(U8, True), bytes_any=True)
row("cvs_link", "block-f32", b_link(F32, True))

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def thresholds(kind, shape):
    """(low, high) for the thinned maps of frame 0 of the contours_batch rows: fractions of their largest response"""
    def make():
        f = cv.SteerableFiltersG2(None) if kind == 2 else cv.SteerableFiltersG4(None, extensions=True)
        outs = f.pipeline(ready(img(shape, 10)))
        hi = max(float(t.max()) for t in f.nonmax(outs[5:8]))
        close(f)
        return (0.2 * hi, 0.5 * hi)
    return cached(("thr", kind, shape), make)


def b_contours_batch(as_block):
    def fn(c, f):
        lo, hi = thresholds(f.KIND, c.shape)
        if as_block:
            x = c.inp(np.stack([img(c.shape, 10 + i) for i in range(3)]), 1)
            out = c.block((3, 3) + c.shape, 2, U8)
            pim, pout, keep, res = f._block_planes(x, 1).ctypes.data_as(L._PP), f._block_planes(out, 2).ctypes.data_as(L._PP), [x, out], [out]
        else:
            xs = [c.inp(img(c.shape, 10 + i)) for i in range(3)]
            res = c.outs([(c.shape, U8)] * 9)
            pim, pout, keep = api._planes(xs), api._planes(res), xs + res
        f._bind_stream(*keep)
        raw(f, "cvs_contours_batch", pim, 3, lo, hi, 2, float("-inf"), pout)
        return res
    return fn


row("cvs_contours_batch", "table-u8", b_contours_batch(False), tags=("strip",), bytes_any=True)
row("cvs_contours_batch", "block-u8", b_contours_batch(True), tags=("strip",), bytes_any=True, host=False)


def labels_of(shape):
    def make():
        f = cv.SteerableFiltersG2(None)
        prep(f, shape, BASIS)
        lab, n = f.label(ready(mask03(shape)))
        res = (lab.cpu().numpy(), n)
        close(f)
        return res
    return cached(("labels", shape), make)


def b_component_stats(c, f):
    prep(f, c.shape, BASIS)
    lab, count = labels_of(c.shape)
    lv, w = c.inp(lab), c.inp(H.make_map(c.shape, 48))
    table = c.array(count * 40, U8)
    f._bind_stream(lv, w)
    pl, pw = P(lv), P(w)
    raw(f, "cvs_component_stats", C.byref(pl), count, C.byref(pw), ptr(table), c.memflag)
    return [table]


row("cvs_component_stats", "table", b_component_stats)


# ---------------------------------------------------------------- lists: arrays with a capacity, called at exactly the capacity the sizing call reports
def chains_of(shape):
    def make():
        f = cv.SteerableFiltersG2(None)
        prep(f, shape, BASIS)
        pts, ch = f.contour_chains(ready(mask03(shape)))
        vt, tab, idx = f.chain_polylines(pts, ch, 1.5, return_index=True)
        masks = torch.stack([ready(mask03(shape, 5 + z)) for z in range(3)])
        bp, bc, br = f.contour_chains_batch(masks)
        res = dict(points=pts.cpu().numpy(), chains=ch.cpu().numpy(), polylines=tab.cpu().numpy(), index=idx.cpu().numpy(),
                   bpoints=bp.cpu().numpy(), branges=br.cpu().numpy())
        close(f)
        return res
    return cached(("chains", shape), make)


def b_contour_points(c, f):
    prep(f, c.shape, BASIS)
    lv = c.inp(labels_of(c.shape)[0])
    f._bind_stream(lv)
    pl, n = P(lv), C.c_int(0)
    assert L.lib().cvs_contour_points(f._h, C.byref(pl), None, 0, c.memflag, C.byref(n)) == L.E_SIZE and n.value > 0
    pts = c.array((n.value, 3), S32)
    raw(f, "cvs_contour_points", C.byref(pl), ptr(pts), n.value, c.memflag, C.byref(n))
    return [pts, np.array([n.value], S32)]


def b_contour_chains(c, f):
    prep(f, c.shape, BASIS)
    m = c.inp(mask03(c.shape))
    f._bind_stream(m)
    pm, n, k = P(m), C.c_int(0), C.c_int(0)
    assert L.lib().cvs_contour_chains(f._h, C.byref(pm), None, 0, None, 0, c.memflag, C.byref(n), C.byref(k)) == L.E_SIZE and n.value and k.value
    pts, ch = c.array((n.value, 2), S32), c.array((k.value, 4), S32)
    raw(f, "cvs_contour_chains", C.byref(pm), ptr(pts), n.value, ptr(ch), k.value, c.memflag, C.byref(n), C.byref(k))
    return [pts, ch, np.array([n.value, k.value], S32)]


def b_chain_polylines(c, f):
    d = chains_of(c.shape)
    pts, ch = c.inp_array(d["points"]), c.inp_array(d["chains"])
    n, m, v = len(d["points"]), len(d["chains"]), C.c_int(0)
    f._bind_stream(pts)
    assert L.lib().cvs_chain_polylines(f._h, ptr(pts), n, ptr(ch), m, 1.5, None, 0, None, None, c.memflag, C.byref(v)) == L.E_SIZE and v.value
    vt, ix, tab = c.array((v.value, 2), S32), c.array(v.value, S32), c.array((m, 4), S32)
    raw(f, "cvs_chain_polylines", ptr(pts), n, ptr(ch), m, 1.5, ptr(vt), v.value, ptr(ix), ptr(tab), c.memflag, C.byref(v))
    return [vt, ix, tab, np.array([v.value], S32)]


def b_chain_refine(c, f):
    """cvs_chain_refine, then cvs_chain_measures and cvs_polyline_segments with caller tables"""
    prep(f, c.shape, BASIS)
    d = chains_of(c.shape)
    mp, th = c.inp(H.make_map(c.shape, 3)), c.inp(H.make_theta(c.shape, 4))
    pts, ch, pl, ix = (c.inp_array(d[k]) for k in ("points", "chains", "polylines", "index"))
    n, m, v = len(d["points"]), len(d["chains"]), len(d["index"])
    xy, st = c.array((n, 2), F32), c.array(n, F32)
    f._bind_stream(mp, th, pts)
    pm, pt = P(mp), P(th)
    raw(f, "cvs_chain_refine", C.byref(pm), C.byref(pt), ptr(pts), n, ptr(xy), ptr(st), c.memflag)
    meas = c.array(m * 40, U8)
    raw(f, "cvs_chain_measures", ptr(pts), n, ptr(ch), m, ptr(xy), ptr(st), ptr(meas), c.memflag)
    seg = c.array(v * 128, U8)
    raw(f, "cvs_polyline_segments", ptr(pts), n, ptr(ch), ptr(pl), m, ptr(ix), v, ptr(xy), ptr(st), ptr(seg), c.memflag)
    return [xy, st, meas, seg]


def b_chains_batch(c, f):
    prep(f, c.shape, BASIS)
    masks = [c.inp(mask03(c.shape, 5 + z)) for z in range(3)]
    f._bind_stream(*masks)
    pm, n, k = api._planes(masks), C.c_int(0), C.c_int(0)
    assert L.lib().cvs_contour_chains_batch(f._h, 3, pm, None, 0, None, 0, None, c.memflag, C.byref(n), C.byref(k)) == L.E_SIZE and n.value and k.value
    pts, ch, rg = c.array((n.value, 2), S32), c.array((k.value, 4), S32), c.array((4, 2), S32)
    raw(f, "cvs_contour_chains_batch", 3, pm, ptr(pts), n.value, ptr(ch), k.value, ptr(rg), c.memflag, C.byref(n), C.byref(k))
    return [pts, ch, rg]


def b_refine_batch(c, f):
    prep(f, c.shape, BASIS)
    d = chains_of(c.shape)
    maps = [c.inp(H.make_map(c.shape, 60 + z)) for z in range(3)]
    ths = [c.inp(H.make_theta(c.shape, 70 + z)) for z in range(3)]
    pts, rg = c.inp_array(d["bpoints"]), c.inp_array(d["branges"])
    n = len(d["bpoints"])
    xy, st = c.array((n, 2), F32), c.array(n, F32)
    f._bind_stream(pts, *maps, *ths)
    raw(f, "cvs_chain_refine_batch", 3, 1, api._planes(maps), api._planes(ths), ptr(pts), n, ptr(rg), ptr(xy), ptr(st), c.memflag)
    return [xy, st]


row("cvs_contour_points", "list", b_contour_points, lists=True)
row("cvs_contour_chains", "list", b_contour_chains, lists=True, bytes_in=True)
row("cvs_chain_polylines", "list", b_chain_polylines, lists=True)
row("cvs_chain_refine", "list-measures-segments", b_chain_refine, lists=True)
row("cvs_contour_chains_batch", "three-planes", b_chains_batch, lists=True, bytes_in=True)
row("cvs_chain_refine_batch", "three-planes", b_refine_batch, lists=True)

for _name in G.COVERED:      # the ledger decides what the table must hold
    if not any(r.entry == _name for r in ROWS):
        raise RuntimeError("tests/roi_guard.py lists %s as COVERED, but the table has no row for it" % _name)
for _r in ROWS:
    if _r.entry not in G.COVERED:
        raise RuntimeError("the table has a row for %s, which roi_guard.COVERED does not list" % _r.entry)
assert len({r.id for r in ROWS}) == len(ROWS)


# ================================================================ the driver
_DENSE = {}


def dense(r, shape, mem):
    """the same call on dense planes of their own, on a fresh handle with the default options; once per (row, shape, memory)"""
    key = (r.id, shape, mem)
    if key not in _DENSE:
        c, f = Ctx(shape, mem, r.make), r.make()
        try:
            res = r.fn(c, f)
            torch.cuda.synchronize()
            _DENSE[key] = [np.ascontiguousarray(G.to_numpy(x)).copy() for x in res]
        finally:
            for h in [f] + c.handles:
                close(h)
    return _DENSE[key]


def drive(r, shape, placement, mem, opts=None, expect=None):
    want = dense(r, shape, mem)
    for surround in (G.BYTE_SURROUNDS if r.bytes_in else (None,)):
        name = "%s %dx%d %s %s%s" % (r.id, shape[0], shape[1], placement, mem, "" if surround is None else " around=0x%02X" % surround)
        c, f = Ctx(shape, mem, r.make, placement, surround), r.make()
        try:
            for o, v in (opts or {}).items():
                f.set_option(o, v)
            res = r.fn(c, f)
            torch.cuda.synchronize()
            G.assert_same_bits(res, want, name)
            for p in c.frames:
                G.assert_frame_intact(p, name)
            for p in c.inputs:
                G.assert_inputs_intact(p, name)
            assert c.frames, name
            if expect:
                info = f.launch_info()
                for k, v in expect.items():
                    assert info[k] == v, (name, k, info)
            for o, v in (opts or {}).items():
                assert f.get_option(o) == v, (name, o)
        finally:
            for h in [f] + c.handles:
                close(h)


def _cases():
    out = []
    for r in ROWS:
        placements = G.PLACEMENTS + (G.BYTE_PLACEMENTS if r.bytes_any else ())
        full = [S1] if r.taps else [S2] if r.lists else [S1, S2]
        small = [] if (r.taps or r.lists) else [FALLBACK[r.kind]] + TINY
        out += [(r, s, p, "dev") for s in full for p in placements]
        out += [(r, s, p, "dev") for s in small for p in ("odd", "tight")]
        if r.host:
            out += [(r, s, p, "host") for s in full for p in ("odd", "wide")]
        if r.lists:     # the input mask, planes and lists keep their bits dense as well as as views
            out += [(r, S2, "odd" + DENSE_IN, mem) for mem in ("dev", "host")]
    return out


def _id(case):
    r, shape, placement, mem = case[:4]
    return "-".join([r.id, "%dx%d" % shape, placement, mem] + [str(x) for x in case[4:]])


CASES = _cases()


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_footprint(case):
    drive(*case)


# ---------------------------------------------------------------- crossed options, at (37, 260), aligned and odd
ORDERS = (L.ORDER_PLAIN, L.ORDER_XCD_COLUMNS, L.ORDER_DYNAMIC_TAIL, -1)   # those of test_block_order_never_changes_results
CROSSED = [(r, S2, p, "dev", name, {opt: v}) for r in ROWS if "strip" in r.tags for p in ("aligned", "odd")
           for name, opt, values in (("order", L.OPT_BLOCK_ORDER, ORDERS), ("strip", L.OPT_STRIP_ROWS, (1, 10, 19, 1000)),
                                     ("layout", L.OPT_STATE_LAYOUT, (0, 1, 2, 3))) for v in values]


@pytest.mark.parametrize("case", CROSSED, ids=[_id(c[:4]) + "-%s=%d" % (c[4], list(c[5].values())[0]) for c in CROSSED])
def test_footprint_under_launch_options(case):
    r, shape, placement, mem, _, opts = case
    drive(r, shape, placement, mem, opts=opts)


NT = [(r, S2, p, "dev") for r in ROWS if ("strip" in r.tags or "point" in r.tags) for p in ("aligned", "odd")]


@pytest.mark.parametrize("case", NT, ids=[_id(c) for c in NT])
def test_footprint_with_streaming_stores(case, monkeypatch):
    """CVS_OPTS=nt_stores=1: the streaming-store instances that otherwise need 2 Mpix"""
    monkeypatch.setenv("CVS_OPTS", "nt_stores=1")
    drive(*case, expect={"nt_stores": 1} if "strip" in case[0].tags else None)


LIT = [(r, S2, p, "dev") for r in ROWS if r.entry == "cvs_pipeline" and not r.taps for p in ("aligned", "odd")]


@pytest.mark.parametrize("case", LIT, ids=[_id(c) for c in LIT])
def test_footprint_with_argument_taps(case, monkeypatch):
    """CVS_OPTS=lit=0: the argument-tap instances of the caller pipeline"""
    monkeypatch.setenv("CVS_OPTS", "lit=0")
    drive(*case, expect={"literal_taps": 0})


# ---------------------------------------------------------------- host planes past the switch to the overlapped host path
OVERLAP = [(r, OVERLAP_SHAPE, "odd", "host", v) for r in ROWS if "overlap" in r.tags for v in (1, 0)]


@pytest.mark.parametrize("case", OVERLAP, ids=[_id(c[:4]) + "-overlap=%d" % c[4] for c in OVERLAP])
def test_footprint_of_the_host_paths_from_1_mpix(case):
    """host views in and out at 1031 x 1019: growing bands on a worker thread (CVS_OPT_HOST_OVERLAP = 1, the default from 2^20 pixels on)
    and one after the other (0); drive() asserts that the option is in effect on the handle that made the call"""
    r, shape, placement, mem, overlap = case
    drive(r, shape, placement, mem, opts={L.OPT_HOST_OVERLAP: overlap})
