"""GPU test (-m gpu): asynchronous calls held to their results while the device runs BEHIND the host (tests/async_gate.py).

Every other GPU test has the device idle when a call is issued, and almost all of them run on the legacy null stream: the library's
ordering mechanisms -- the event of cvs_set_stream, the `ready` event of a parked state block, the reset of a recycled tile-queue slot,
the sync-then-free of handle scratch, the streams of the host path, the tuner's events, the synchronize() of batch.py -- are executed
there and verified nowhere.  Here every section runs on a non-blocking side stream behind a bounded delay, its inputs hold poison (NaN /
0xA5) until a copy BEHIND the delay gives them their values, and its outputs start as a sentinel.

Reference of every comparison: the QUIET TWIN -- the same body of code on a fresh handle with every input ready and a synchronize()
after every call -- bit for bit.  (The twin is what the existing tests pin to the oracle and the models.)  Nothing is compared with a
gated run of itself.

Scenarios (the section names in failures):
  A  late inputs, one call family per section; the calls include/cvsteer_hip.h documents as asynchronous also assert the PREMISE
     still_gated() after the last call returned: they were queued while the device was behind and none of them waited on the host
  B  calls that synchronise: the values they return to the host are right at return, with no sync of the test's own
  C  whole dependent chains behind one gate, the tail twice back to back
  D  stream hops (cvs_set_stream), also with the handle's first-ever call on the second stream
  E  state blocks handed over by the pool with the previous owner's work pending
  F  scratch growth under load      G  the tuner on a deep queue      H  the synchronize() of NativeBatch.run
The positive control shows on the machine, with torch alone, that a missing wait IS visible at the delay used.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import async_gate as G
import cvsteer_amd as cv
import handle_sequences as H
from cvsteer_amd import _lib as L
from cvsteer_amd import batch
from cvsteer_amd.api import _plane as P
from helpers import EDGE_SHAPES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL, LARGE = (70, 129), (185, 256)
assert SMALL in EDGE_SHAPES and LARGE in EDGE_SHAPES
BASIS, FULL = cv.SETUP_BASIS, cv.SETUP_FULL
LOW, HIGH = H.LOW, H.HIGH            # for maps that are uniform on [0, 1)
ANGLES = [0.3, -1.1, 2.0]
_STREAMS = []


def S(i):
    """non-blocking side streams"""
    while len(_STREAMS) <= i:
        _STREAMS.append(torch.cuda.Stream(DEV))
    return _STREAMS[i]


def mk(kind):
    return cv.SteerableFiltersG2(None) if kind == 2 else cv.SteerableFiltersG4(None, extensions=True)


def close(f):
    f.__del__()


def img(shape, seed):
    return H.make_image((shape[0], shape[1], seed, False))


def ready(a):
    """a device tensor whose values have landed"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def to_np(x):
    if torch.is_tensor(x):
        return x.detach().cpu().numpy()
    a = np.asarray(x)
    return np.frombuffer(a.tobytes(), np.uint8) if a.dtype.names else a


def raw(f, name, *args):
    rc = getattr(L.lib(), name)(f._h, *args)
    if rc:
        raise cv.CvsError(rc, name, L.lib().cvs_last_error(f._h).decode())


def snap(f):
    """every state plane of the selected frame: (status, values)"""
    out = []
    for code in list(range(H.NB[f.KIND])) + [L.PLANE_C1, L.PLANE_C2, L.PLANE_C3, L.PLANE_THETA, L.PLANE_STRENGTH]:
        try:
            out.append((0, to_np(f._state(code))))
        except cv.CvsError as e:
            out.append((e.status, None))
    return out


def check(name, got, want):
    assert len(got) == len(want), (name, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, "%s: result %d is %s %s, the quiet twin's %s %s" % (name, k, g.shape, g.dtype, w.shape, w.dtype)
        if g.tobytes() != w.tobytes():
            bad = int(np.count_nonzero(g.reshape(-1).view(np.uint8) != w.reshape(-1).view(np.uint8)))
            nan = int(np.isnan(g).sum()) if g.dtype.kind == "f" else 0
            sent = int((g == G.SENTINEL_F32).sum()) if g.dtype.kind == "f" else int((g.reshape(-1).view(np.uint8) == G.SENTINEL_BYTE).sum())
            raise AssertionError("%s: result %d differs from the quiet twin in %d of %d bytes (%d NaN, %d sentinel values in it)"
                                 % (name, k, bad, g.nbytes, nan, sent))


def check_state(name, got, want):
    assert [s for s, _ in got] == [s for s, _ in want], (name, [s for s, _ in got], [s for s, _ in want])
    check(name + " state planes", [a for s, a in got if s == 0], [a for s, a in want if s == 0])


def run_case(case, kind, shape, stream=None, premise=True, ms=G.START_MS, name=""):
    """the quiet twin on a fresh handle; then a second handle: warmed by the same body on OTHER inputs (state and scratch exist, code
    objects are loaded: the asserted pass allocates nothing), and the gated pass"""
    stream = stream or S(0)
    name = name or "%s G%d %dx%d" % (case.__name__, kind, shape[0], shape[1])
    with torch.cuda.stream(stream):
        tw = mk(kind)
        sec = G.Section(stream, ms, "quiet", name)
        want = [to_np(x) for x in case(tw, sec, shape, 1)]
        sec.finish()
        wstate = snap(tw)
        close(tw)
        f = mk(kind)
        sec = G.Section(stream, ms, "quiet", name)
        case(f, sec, shape, 2)
        sec.finish()
        sec = G.behind(stream, ms, name)
        res = case(f, sec, shape, 1)
        if premise:
            sec.premise()
        sec.finish()
        got = [to_np(x) for x in res]
        gstate = snap(f)
        close(f)
    check(name, got, want)
    check_state(name, gstate, wstate)


_THR = {}


def thr(kind, shape):
    """(largest thinned find(magnitude) response, largest thinned find(e) response) of image 1: thresholds are fractions of them"""
    key = (kind, shape)
    if key not in _THR:
        f = mk(kind)
        outs = f.pipeline(ready(img(shape, 1)))
        hi_m = max(float(t.max()) for t in f.nonmax(outs[5:8]))
        hi_e = max(float(t.max()) for t in f.nonmax(f.find(outs[2], outs[4])))
        torch.cuda.synchronize()
        close(f)
        assert hi_m > 0.0 and hi_e > 0.0
        _THR[key] = (hi_m, hi_e)
    return _THR[key]


def half(shape):
    return ((shape[0] + 1) // 2, (shape[1] + 1) // 2)


def pre_setup(f, shape, seed, flags=None):
    """quiet preamble of a section: image size and state from a ready image"""
    f.setup(ready(img(shape, 100 + seed)), flags)


def padded(sec, shape, k, dtype=np.float32):
    """an output plane in an allocation of its own with a row pitch of its own: no constant distance, no common step"""
    return sec.out((shape[0], shape[1] + 4 + 4 * (k % 2)), dtype)[:, :shape[1]]


def raw_find(f, e, ph, outs):
    f._bind_stream(e, ph, *outs)
    pe, pp, po = P(e), P(ph), [P(o) for o in outs]
    raw(f, "cvs_find", C.byref(pe), C.byref(pp), *[C.byref(p) for p in po])


def raw_contours_batch(f, frames, low, high, min_area, min_peak, out):
    pim, pout = f._block_planes(frames, 1), f._block_planes(out, 2)
    f._like = frames[0]
    f._bind_stream(frames, out)
    raw(f, "cvs_contours_batch", pim.ctypes.data_as(L._PP), int(frames.shape[0]), float(low), float(high), int(min_area), float(min_peak),
        pout.ctypes.data_as(L._PP))
    f._batch_keepalive = (frames, out)


def chain_table(n):
    """two chains over n points: an open one and a closed one"""
    return np.array([[0, 10, 0, 0], [10, n - 10, L.CHAIN_CLOSED, 0]], np.int32)


def batch_points(shape, seed, planes, per=10):
    """points and the range table of cvs_contour_chains_batch for `planes` planes of `per` points each"""
    pts = np.concatenate([H.make_points(shape, seed + z, per) for z in range(planes)])
    rng = np.array([[z, per * z] for z in range(planes + 1)], np.int32)
    return pts, rng


# ================================================================ A: late inputs, one call family per section
def a_setup_basis(f, sec, shape, seed):
    x = sec.inp(img(shape, seed))
    sec.start()
    f.setup(x, BASIS)
    sec.step()
    return []


def a_setup_full(f, sec, shape, seed):
    x = sec.inp(img(shape, seed))
    sec.start()
    f.setup(x, FULL)
    sec.step()
    return []


def a_setup_steer(f, sec, shape, seed):
    x, g, h = sec.inp(img(shape, seed)), sec.out(shape), sec.out(shape)
    sec.start()
    f.setup_steer(x, 0.7, BASIS, out=(g, h))
    sec.step()
    return [g, h]


def a_setup_rows(f, sec, shape, seed):
    flags = FULL if f.KIND == 2 else BASIS   # (the header: no orientation bands for G4)
    pre_setup(f, shape, seed, flags)
    x = sec.inp(img(shape, seed))
    sec.start()
    f._bind_stream(x)
    p = P(x)
    raw(f, "cvs_setup_rows", C.byref(p), flags, 20, 45)
    f._image_keepalive = x
    sec.step()
    return []


def a_setup_pyr(f, sec, shape, seed):
    x, nxt = sec.inp(img(shape, seed)), sec.out(half(shape))
    sec.start()
    f.setup_pyr(x, out=nxt)
    sec.step()
    return [nxt]


def a_pyr_down(f, sec, shape, seed):
    x, dst = sec.inp(img(shape, seed)), sec.out(half(shape))
    sec.start()
    f._bind_stream(x, dst)
    ps, pd = P(x), P(dst)
    raw(f, "cvs_pyr_down", C.byref(ps), C.byref(pd))
    sec.step()
    return [dst]


def _late_setup(f, sec, x, flags=FULL):
    sec.start()
    f.setup(x, flags)
    sec.step()


def a_steer_scalar(f, sec, shape, seed):
    x, outs = sec.inp(img(shape, seed)), [sec.out(shape) for _ in range(5)]
    _late_setup(f, sec, x)
    f.steer(0.4, True, out=outs)
    sec.step()
    return outs


def a_steer_map_own_theta(f, sec, shape, seed):
    x, outs = sec.inp(img(shape, seed)), [sec.out(shape) for _ in range(5)]
    _late_setup(f, sec, x)
    f.steer(None, True, out=outs)
    sec.step()
    return outs


def a_steer_map_late_theta(f, sec, shape, seed):
    x, th, outs = sec.inp(img(shape, seed)), sec.inp(H.make_theta(shape, seed)), [sec.out(shape) for _ in range(5)]
    _late_setup(f, sec, x)
    f.steer(th, True, out=outs)
    sec.step()
    return outs


def a_steer_bank_block(f, sec, shape, seed):
    x, blk = sec.inp(img(shape, seed)), sec.out((5, len(ANGLES)) + shape)
    _late_setup(f, sec, x)
    f.steer_bank(ANGLES, full=True, out=[blk[i] for i in range(5)])
    sec.step()
    return [blk]


def a_orientation_peaks_block(f, sec, shape, seed):
    x, blk, cnt = sec.inp(img(shape, seed)), sec.out((2, 2) + shape), sec.out(shape, np.uint8)
    _late_setup(f, sec, x, BASIS)
    f.orientation_peaks(n_angles=16, max_peaks=2, out=(blk[0], blk[1], cnt))
    sec.step()
    return [blk, cnt]


def a_mag_phase(f, sec, shape, seed):
    pre_setup(f, shape, seed)
    g, h = sec.inp(H.make_map(shape, seed) - np.float32(0.5)), sec.inp(H.make_map(shape, seed + 1) - np.float32(0.5))
    m, ph = sec.out(shape), sec.out(shape)
    sec.start()
    f._bind_stream(g, h, m, ph)
    pg, phh, pm, pp = P(g), P(h), P(m), P(ph)
    raw(f, "cvs_mag_phase", C.byref(pg), C.byref(phh), C.byref(pm), C.byref(pp))
    sec.step()
    return [m, ph]


def a_wrap(f, sec, shape, seed):
    pre_setup(f, shape, seed)
    a, o = sec.inp(H.make_theta(shape, seed) * np.float32(3.0)), sec.out(shape)
    sec.start()
    f._bind_stream(a, o)
    pa, po = P(a), P(o)
    raw(f, "cvs_wrap", C.byref(pa), C.byref(po))
    sec.step()
    return [o]


def a_phase_weights(f, sec, shape, seed):
    pre_setup(f, shape, seed)
    ph, lam = sec.inp(H.make_theta(shape, seed) * np.float32(2.0)), sec.out(shape)
    sec.start()
    f._bind_stream(ph, lam)
    pp, pl = P(ph), P(lam)
    raw(f, "cvs_phase_weights", C.byref(pp), C.byref(pl), 0.5, 1, 2.0)
    sec.step()
    return [lam]


def a_find(f, sec, shape, seed):
    pre_setup(f, shape, seed)
    e, ph = sec.inp(H.make_map(shape, seed)), sec.inp(H.make_theta(shape, seed) * np.float32(2.0))
    outs = [sec.out(shape) for _ in range(3)]
    sec.start()
    raw_find(f, e, ph, outs)
    sec.step()
    return outs


def a_pipeline(f, sec, shape, seed):
    x, outs = sec.inp(img(shape, seed)), [sec.out(shape) for _ in range(8)]
    sec.start()
    f.pipeline(x, out=outs)
    sec.step()
    return outs


def a_pipeline_batch_regular_select_frame(f, sec, shape, seed):
    fr, out = sec.inp(np.stack([img(shape, seed + 10 * i) for i in range(3)])), sec.out((3, 8) + shape)
    sec.start()
    f.pipeline_batch(fr, out=out)
    sec.step()
    f.select_frame(2)
    return [out]


def a_pipeline_batch_irregular(f, sec, shape, seed):
    """frames in allocations of their own with two row pitches: the launch reads them through the handle's frame table"""
    frames = []
    for i in range(3):
        a = np.zeros((shape[0], shape[1] + 4 + 4 * (i % 2)), np.float32)
        a[:, :shape[1]] = img(shape, seed + 10 * i)
        frames.append(sec.inp(a)[:, :shape[1]])
    out = sec.out((3, 8) + shape)
    sec.start()
    f.pipeline_batch(frames, out=out)
    sec.step()
    f.select_frame(1)
    return [out]


def a_nonmax(f, sec, shape, seed):
    pre_setup(f, shape, seed)
    maps, th = [sec.inp(H.make_map(shape, seed + k)) for k in range(3)], sec.inp(H.make_theta(shape, seed))
    outs = [sec.out(shape) for _ in range(3)]
    sec.start()
    f.nonmax(maps, theta=th, out=outs)
    sec.step()
    return outs


def a_nonmax_batch(f, sec, shape, seed):
    pre_setup(f, shape, seed)
    maps = sec.inp(H.make_map((2, 3) + shape, seed))
    th, out = sec.inp(np.stack([H.make_theta(shape, seed + i) for i in range(2)])), sec.out((2, 3) + shape)
    sec.start()
    f.nonmax_batch(maps, theta=th, out=out)
    sec.step()
    return [out]


def a_link(f, sec, shape, seed):
    pre_setup(f, shape, seed)
    maps, out = sec.inp(H.make_map((3,) + shape, seed)), sec.out((3,) + shape, np.uint8)
    sec.start()
    f.link(maps, LOW, HIGH, min_area=2, out=out)
    sec.step()
    return [out]


def a_contours_batch(f, sec, shape, seed):
    hi = thr(f.KIND, shape)[0]
    fr, out = sec.inp(np.stack([img(shape, seed + 10 * i) for i in range(2)])), sec.out((2, 3) + shape, np.uint8)
    sec.start()
    raw_contours_batch(f, fr, 0.05 * hi, 0.2 * hi, 2, -np.inf, out)
    sec.step()
    if not sec.gated and seed == 1:
        assert 0 < int((out == 255).sum()) < out.numel()
    return [out]


def a_chain_refine(f, sec, shape, seed):
    pre_setup(f, shape, seed)
    pts, m, th = sec.inp(H.make_points(shape, seed)), sec.inp(H.make_map(shape, seed)), sec.inp(H.make_theta(shape, seed))
    xy, st = sec.out((37, 2)), sec.out((37,))
    sec.start()
    f.chain_refine(pts, m, theta=th, out=(xy, st))
    sec.step()
    return [xy, st]


def a_chain_refine_batch(f, sec, shape, seed):
    pre_setup(f, shape, seed)
    p, r = batch_points(shape, seed, 6)
    pts, rng = sec.inp(p), sec.inp(r)
    maps = sec.inp(H.make_map((2, 3) + shape, seed))
    th = sec.inp(np.stack([H.make_theta(shape, seed + i) for i in range(2)]))
    xy, st = sec.out((60, 2)), sec.out((60,))
    sec.start()
    f.chain_refine_batch(pts, rng, maps, theta=th, out=(xy, st))
    sec.step()
    return [xy, st]


def a_chain_measures(f, sec, shape, seed):
    pts, ch = sec.inp(H.make_points(shape, seed)), sec.inp(chain_table(37))
    st, xy = sec.inp(H.make_map((37,), seed)), sec.inp(H.make_map((37, 2), seed) * np.float32(50.0))
    out = sec.out((2, 40), np.uint8)
    sec.start()
    f.chain_measures(pts, ch, strength=st, xy=xy, out=out)
    sec.step()
    return [out]


def _u8_outs(sec, shape, which):
    return [sec.out(shape, np.uint8) if k in which else None for k in range(8)]


def a_pipeline_u8_all_outputs(f, sec, shape, seed):
    """8-bit device outputs with state kept: the f32 maps go through the handle's u8 scratch, then the quantise kernels"""
    x, outs = sec.inp(img(shape, seed)), _u8_outs(sec, shape, range(8))
    sec.start()
    f.pipeline(x, out=outs)
    sec.step()
    return outs


def _three_maps(f, sec, shape, seed, gain):
    f.set_persist(False)
    f.set_u8_gain(gain)
    x, outs = sec.inp(img(shape, seed)), _u8_outs(sec, shape, (5, 6, 7))
    sec.start()
    f.pipeline(x, out=outs)
    sec.step()
    return outs[5:8]


def a_pipeline_u8_three_maps_normalise(f, sec, shape, seed):
    """the three maps as bytes, no state: min / max in the filter launch (or after it), then the quantise launch"""
    return _three_maps(f, sec, shape, seed, 0.0)


def a_pipeline_u8_three_maps_gain(f, sec, shape, seed):
    return _three_maps(f, sec, shape, seed, 3.0)


def a_pipeline_batch_u8(f, sec, shape, seed):
    fr, out = sec.inp(np.stack([img(shape, seed + 10 * i) for i in range(3)])), sec.out((3, 8) + shape, np.uint8)
    sec.start()
    f.pipeline_batch(fr, out=out)
    sec.step()
    f.select_frame(1)
    return [out]


def a_pipeline_batch_u8_three_maps(f, sec, shape, seed):
    f.set_persist(False)
    fr, out = sec.inp(np.stack([img(shape, seed + 10 * i) for i in range(3)])), sec.out((3, 3) + shape, np.uint8)
    sec.start()
    f.pipeline_batch(fr, out=out, outputs=[5, 6, 7])
    sec.step()
    return [out]


def a_normalize_u8(f, sec, shape, seed):
    m, dst = sec.inp(H.make_map(shape, seed)), sec.out(shape, np.uint8)
    sec.start()
    f._bind_stream(m, dst)
    pm = P(m)
    raw(f, "cvs_normalize_u8", C.byref(pm), C.c_void_p(dst.data_ptr()), dst.stride(0), L.MEM_DEVICE)
    sec.step()
    return [dst]


def a_convert_u8(f, sec, shape, seed):
    m, dst = sec.inp(H.make_map(shape, seed)), sec.out(shape, np.uint8)
    sec.start()
    f._bind_stream(m, dst)
    pm = P(m)
    raw(f, "cvs_convert_u8", C.byref(pm), 200.0, 3.0, C.c_void_p(dst.data_ptr()), dst.stride(0), L.MEM_DEVICE)
    sec.step()
    return [dst]


def _u8_batch(f, sec, shape, seed, normalise, block):
    """n planes at once: one block in and out (one launch pair), or planes in allocations of their own (plane by plane)"""
    n = 3
    if block:
        m, dst = sec.inp(H.make_map((n,) + shape, seed)), sec.out((n,) + shape, np.uint8)
        src, dsts = [m[i] for i in range(n)], [dst[i] for i in range(n)]
    else:
        src = []
        for i in range(n):
            a = np.zeros((shape[0], shape[1] + 4 + 4 * (i % 2)), np.float32)
            a[:, :shape[1]] = H.make_map(shape, seed + i)
            src.append(sec.inp(a)[:, :shape[1]])
        dsts = [sec.out(shape, np.uint8) for _ in range(n)]
    sec.start()
    f._bind_stream(*src, *dsts)
    planes = (L.Plane * n)(*[P(t) for t in src])
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in dsts])
    if normalise:
        raw(f, "cvs_normalize_u8_batch", planes, n, ptrs, shape[1], L.MEM_DEVICE)
    else:
        raw(f, "cvs_convert_u8_batch", planes, n, 200.0, 3.0, ptrs, shape[1], L.MEM_DEVICE)
    sec.step()
    return dsts


def a_normalize_u8_batch_block(f, sec, shape, seed):
    return _u8_batch(f, sec, shape, seed, True, True)


def a_normalize_u8_batch_scattered(f, sec, shape, seed):
    return _u8_batch(f, sec, shape, seed, True, False)


def a_convert_u8_batch_block(f, sec, shape, seed):
    return _u8_batch(f, sec, shape, seed, False, True)


def a_convert_u8_batch_scattered(f, sec, shape, seed):
    return _u8_batch(f, sec, shape, seed, False, False)


def a_read_state_device(f, sec, shape, seed):
    """cvs_read_state into device planes: a copy on the handle's stream, no sync"""
    x = sec.inp(img(shape, seed))
    dsts = [sec.out(shape), padded(sec, shape, 1)]
    _late_setup(f, sec, x)
    for which, d in zip((L.PLANE_BASIS0 + 2, L.PLANE_THETA), dsts):
        p = P(d)
        raw(f, "cvs_read_state", which, C.byref(p))
    sec.step()
    return dsts


def a_pyramid_setup(f, sec, shape, seed):
    """cvs_pyramid_setup on device planes: three handles, three levels, one chain of launches; the state of every level is read
    back into device planes behind it (cvs_read_state, asynchronous as well)"""
    if not hasattr(f, "_levels"):
        f._levels = [f] + [mk(f.KIND) for _ in range(2)]
    hs = f._levels
    shapes = [shape, half(shape), half(half(shape))]
    x, levels = sec.inp(img(shape, seed)), [sec.out(shapes[1]), sec.out(shapes[2])]
    planes = [sec.out(sh) for sh in shapes]
    sec.start()
    cv.api.pyramid_setup(hs, x, level_images=levels, flags=BASIS)
    sec.step()
    for hnd, d in zip(hs, planes):
        p = P(d)
        raw(hnd, "cvs_read_state", L.PLANE_BASIS0 + 1, C.byref(p))
    sec.step()
    return levels + planes


G2_ONLY = (a_wrap, a_phase_weights)   # (entry points of the G2 class alone)
A_CASES = [a_setup_basis, a_setup_full, a_setup_steer, a_setup_rows, a_setup_pyr, a_pyr_down, a_steer_scalar, a_steer_map_own_theta,
           a_steer_map_late_theta, a_steer_bank_block, a_orientation_peaks_block, a_mag_phase, a_wrap, a_phase_weights, a_find, a_pipeline,
           a_pipeline_batch_regular_select_frame, a_pipeline_batch_irregular, a_nonmax, a_nonmax_batch, a_link, a_contours_batch,
           a_chain_refine, a_chain_refine_batch, a_chain_measures,
           # the rest of what the header's general rule covers ("calls with only DEVICE planes are asynchronous")
           a_pipeline_u8_all_outputs, a_pipeline_u8_three_maps_normalise, a_pipeline_u8_three_maps_gain, a_pipeline_batch_u8,
           a_pipeline_batch_u8_three_maps, a_normalize_u8, a_convert_u8, a_normalize_u8_batch_block, a_normalize_u8_batch_scattered,
           a_convert_u8_batch_block, a_convert_u8_batch_scattered, a_read_state_device, a_pyramid_setup]
KIND_SHAPE = [(2, SMALL), (2, LARGE), (4, SMALL), (4, LARGE)]
KIND_SHAPE_IDS = ["g2_small", "g2_large", "g4_small", "g4_large"]


def _cases(cases, g2_only):
    return [pytest.param(c, k, sh, id="%s-%s" % (c.__name__, i)) for c in cases for (k, sh), i in zip(KIND_SHAPE, KIND_SHAPE_IDS)
            if k == 2 or c not in g2_only]


@pytest.mark.parametrize("case,kind,shape", _cases(A_CASES, G2_ONLY))
def test_a_late_inputs(case, kind, shape):
    """(A) asynchronous by the header: queued behind the gate, not waited for, and right once the stream has drained.  70 x 129 and
    185 x 256, G2 and G4 (the entry points of the G2 class alone: G2)"""
    run_case(case, kind, shape)


def test_a_late_inputs_on_the_default_stream():
    """(A) the same on the legacy null stream, where every other test of the suite runs"""
    run_case(a_pipeline, 2, SMALL, stream=torch.cuda.default_stream(DEV), name="a_pipeline on the default stream")


def test_positive_control_a_missing_wait_is_visible_at_this_delay():
    """torch only, no library code, valid memory only: behind a gate on S1 a tensor gets its values late; a read on a second non-blocking
    stream WITHOUT a wait sees the poison, the same read after S2.wait_stream(S1) sees the values"""
    s1, s2 = S(0), S(1)
    data = np.arange(4096, dtype=np.float32)
    sec = G.behind(s1, name="positive control")
    dst = sec.inp(data)
    sec.start()
    with torch.cuda.stream(s2):
        early = dst.clone()
    s2.synchronize()
    assert sec.still_gated(), "the delay of %g ms had passed before the unordered read was made" % sec.ms
    with torch.cuda.stream(s2):
        s2.wait_stream(s1)
        ordered = dst.clone()
    s2.synchronize()
    assert not sec.still_gated()
    sec.finish()
    cal = G.calibrate(DEV)
    print("positive control: %s per ms = %.1f, calibration delay realised %.2f ms, gate %g ms" % (cal["unit"], cal["cycles_per_ms"], cal["realised_ms"], sec.ms))
    assert bool(torch.isnan(early).all()), "the unordered read did not see the poison"
    assert np.array_equal(ordered.cpu().numpy(), data)


def test_realised_gate_delay():
    """the delay a gate realises, measured between two events around it (printed; the bound is loose: the premise checks are what hold
    every section to its delay)"""
    s = S(0)
    e0 = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        e0.record(s)
    G.gate(s, G.START_MS)
    e1 = torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        e1.record(s)
    e1.synchronize()
    ms = e0.elapsed_time(e1)
    print("gate(%g ms) realised %.2f ms" % (G.START_MS, ms))
    assert 0.5 * G.START_MS <= ms <= 4.0 * G.START_MS
    with pytest.raises(ValueError):
        G.gate(s, 251.0)


# ================================================================ B: synchronising calls behind a gate
def b_hysteresis(f, sec, shape, seed):
    pre_setup(f, shape, seed)
    maps, outs = [sec.inp(H.make_map(shape, seed + k)) for k in range(2)], [sec.out(shape, np.uint8) for _ in range(2)]
    sec.start()
    _, passes = f.hysteresis(maps, LOW, HIGH, out=outs, return_passes=True)
    return [np.int64(passes)] + outs


def b_label(f, sec, shape, seed):
    pre_setup(f, shape, seed)
    mask, lab = sec.inp(H.make_mask(shape, seed, False)), sec.out(shape, np.int32)
    sec.start()
    _, count = f.label(mask, out=lab)
    return [np.int64(count), lab]


def _quiet_labels(f, shape, seed):
    lab, count = f.label(ready(H.make_mask(shape, seed, False)))
    return lab.cpu().numpy(), count


def b_component_stats(f, sec, shape, seed):
    pre_setup(f, shape, seed)
    labels, count = _quiet_labels(f, shape, seed)
    lab, w = sec.inp(labels), sec.inp(H.make_map(shape, seed))
    sec.start()
    return [f.component_stats(lab, count, weight=w)]


def b_contour_prune(f, sec, shape, seed):
    pre_setup(f, shape, seed)
    masks = [sec.inp(H.make_mask(shape, seed + k, False)) for k in range(2)]
    ws, outs = [sec.inp(H.make_map(shape, seed + k)) for k in range(2)], [sec.out(shape, np.uint8) for _ in range(2)]
    sec.start()
    _, kept = f.prune(masks, 3, weight=ws, min_peak=0.5, out=outs, return_kept=True)
    return [np.array(kept, np.int64)] + outs


def b_contour_points(f, sec, shape, seed):
    pre_setup(f, shape, seed)
    lab = sec.inp(_quiet_labels(f, shape, seed)[0])
    sec.start()
    return [f.contour_points(lab)]   # the sizing call and the filling call


def b_contour_chains(f, sec, shape, seed):
    pre_setup(f, shape, seed)
    mask = sec.inp(H.make_mask(shape, seed, False))
    sec.start()
    return list(f.contour_chains(mask))   # the sizing call and the filling call


def b_contour_chains_batch(f, sec, shape, seed):
    pre_setup(f, shape, seed)
    masks = sec.inp(np.stack([H.make_mask(shape, seed + k, False) for k in range(2)]))
    sec.start()
    return list(f.contour_chains_batch(masks))


def b_chain_polylines(f, sec, shape, seed):
    pre_setup(f, shape, seed)
    p, c = f.contour_chains(ready(H.make_mask(shape, seed, False)))
    pts, ch = sec.inp(p.cpu().numpy()), sec.inp(c.cpu().numpy())
    sec.start()
    return list(f.chain_polylines(pts, ch, 1.0, return_index=True))


def b_steer_point(f, sec, shape, seed):
    x = sec.inp(img(shape, seed))
    _late_setup(f, sec, x)
    return [np.array(f.steer_point((5, 7), 0.3, full=True), np.float32)]


def b_read_state_host(f, sec, shape, seed):
    x = sec.inp(img(shape, seed))
    _late_setup(f, sec, x)
    res = []
    for which in (L.PLANE_BASIS0 + 2, L.PLANE_THETA):
        host = G.sentinel(shape, np.float32)
        p = P(host)
        raw(f, "cvs_read_state", which, C.byref(p))
        res.append(host.copy())   # as it is at return
    return res


def b_steer_bank_staged(f, sec, shape, seed):
    x = sec.inp(img(shape, seed))
    outs = [[padded(sec, shape, k) for k in range(len(ANGLES))] for _ in range(5)]
    _late_setup(f, sec, x)
    f.steer_bank(ANGLES, full=True, out=outs)
    return [o for kind in outs for o in kind]


def b_orientation_peaks_staged(f, sec, shape, seed):
    x = sec.inp(img(shape, seed))
    ang, en, cnt = [padded(sec, shape, k) for k in range(2)], [padded(sec, shape, k + 1) for k in range(2)], sec.out(shape, np.uint8)
    _late_setup(f, sec, x, BASIS)
    f.orientation_peaks(n_angles=12, max_peaks=2, out=(ang, en, cnt))
    return ang + en + [cnt]


def b_late_device_theta_host_outputs(f, sec, shape, seed):
    x, th = sec.inp(img(shape, seed)), sec.inp(H.make_theta(shape, seed))
    _late_setup(f, sec, x)
    outs = [G.sentinel(shape, np.float32) for _ in range(5)]
    f.steer(th, True, out=outs)
    return [o.copy() for o in outs]   # as they are at return


def b_host_image_behind_pending_device_work(f, sec, shape, seed):
    """a host image of 1 Mpix and more with host outputs: the overlapped up and down streams and the download thread run while the
    gated device call of the same handle is still pending"""
    x, douts = sec.inp(img(shape, seed)), [sec.out(shape) for _ in range(8)]
    sec.start()
    f.pipeline(x, out=douts)
    sec.step()
    houts = [G.sentinel(shape, np.float32) for _ in range(8)]
    f.pipeline(img(shape, seed + 50), out=houts)
    return [o.copy() for o in houts] + douts


B_CASES = [b_hysteresis, b_label, b_component_stats, b_contour_prune, b_contour_points, b_contour_chains, b_contour_chains_batch,
           b_chain_polylines, b_steer_point, b_read_state_host, b_steer_bank_staged, b_orientation_peaks_staged,
           b_late_device_theta_host_outputs]


# staged placements on the device: the launch writes a block of the arena and device-to-device copies carry the planes out, all on the
# handle's stream -- cvs_api.cpp / cvs_peaks.cpp synchronise only when a plane is a host plane, so these two hold the premise as well
B_ASYNC = (b_steer_bank_staged, b_orientation_peaks_staged)


@pytest.mark.parametrize("case,kind,shape", _cases(B_CASES, (b_steer_point,)))
def test_b_synchronising_calls(case, kind, shape):
    """(B) the late inputs are on the handle's stream; what the call hands to the host is right when it returns.  70 x 129 and
    185 x 256, G2 and G4 (cvs_steer_point: G2)"""
    run_case(case, kind, shape, premise=case in B_ASYNC)


@pytest.mark.parametrize("kind", [2, 4])
def test_b_host_image_behind_pending_device_work(kind):
    run_case(b_host_image_behind_pending_device_work, kind, (1024, 1040), premise=False)


# ================================================================ C: chains without a sync
def c_chain_single(f, sec, shape, seed):
    """setup -> steer (own theta, full) -> find -> [nonmax -> link -> chain_refine -> chain_measures] twice: on find(magnitude) and on
    find(e), the second tail queued while the first still is"""
    hi = thr(f.KIND, shape)
    x = sec.inp(img(shape, seed))
    ch = sec.inp(chain_table(37))
    st5 = [sec.out(shape) for _ in range(5)]
    res = list(st5)
    tails = []
    for t in range(2):
        tails.append(dict(pts=sec.inp(H.make_points(shape, seed + 7 * t)), maps=[sec.out(shape) for _ in range(3)], thin=sec.out((3,) + shape),
                          mask=sec.out((3,) + shape, np.uint8), xy=sec.out((37, 2)), st=sec.out((37,)), tab=sec.out((2, 40), np.uint8)))
    sec.start()
    f.setup(x, FULL)
    sec.step()
    f.steer(None, True, out=st5)
    sec.step()
    for t, T in enumerate(tails):
        raw_find(f, st5[3] if t == 0 else st5[2], st5[4], T["maps"])
        sec.step()
        f.nonmax(T["maps"], out=[T["thin"][k] for k in range(3)])
        sec.step()
        f.link(T["thin"], 0.05 * hi[t], 0.2 * hi[t], min_area=2, out=T["mask"])
        sec.step()
        f.chain_refine(T["pts"], T["maps"][0], out=(T["xy"], T["st"]))
        sec.step()
        f.chain_measures(T["pts"], ch, strength=T["st"], xy=T["xy"], out=T["tab"])
        sec.step()
        res += T["maps"] + [T["thin"], T["mask"], T["xy"], T["st"], T["tab"]]
    return res


def c_chain_batch(f, sec, shape, seed):
    """[pipeline_batch -> nonmax_batch -> contours_batch -> chain_refine_batch] twice on other frames"""
    hi = thr(f.KIND, shape)[0]
    res, runs = [], []
    for t in range(2):
        p, r = batch_points(shape, seed + 3 * t, 6)
        runs.append(dict(fr=sec.inp(np.stack([img(shape, seed + 10 * i + 5 * t) for i in range(2)])), maps=sec.out((2, 3) + shape),
                         thin=sec.out((2, 3) + shape), mask=sec.out((2, 3) + shape, np.uint8), pts=sec.inp(p), rng=sec.inp(r),
                         xy=sec.out((60, 2)), st=sec.out((60,))))
    sec.start()
    for R in runs:
        f.pipeline_batch(R["fr"], out=R["maps"], outputs=[5, 6, 7])
        sec.step()
        f.nonmax_batch(R["maps"], out=R["thin"])
        sec.step()
        raw_contours_batch(f, R["fr"], 0.05 * hi, 0.2 * hi, 2, -np.inf, R["mask"])
        sec.step()
        f.chain_refine_batch(R["pts"], R["rng"], R["maps"], out=(R["xy"], R["st"]))
        sec.step()
        res += [R["maps"], R["thin"], R["mask"], R["xy"], R["st"]]
    return res


@pytest.mark.parametrize("case", [c_chain_single, c_chain_batch], ids=lambda c: c.__name__)
@pytest.mark.parametrize("kind,shape", [(2, SMALL), (4, LARGE), (2, LARGE)])
def test_c_chains_without_a_sync(case, kind, shape):
    """(C) one gate, the whole dependent sequence, one sync at the end; every call of it is asynchronous by the header"""
    run_case(case, kind, shape)


# ================================================================ D: stream hops
def _d_setup_bank(shape):
    def inputs(seed):
        return img(shape, seed)

    def call1(f, x, o1):
        f.setup(x, FULL)

    def call2(f, o2):
        f.steer_bank(ANGLES, full=True, out=[o2[0][i] for i in range(5)])
    return inputs, (lambda sec: []), (lambda sec: [sec.out((5, len(ANGLES)) + shape)]), call1, call2


def _d_pipeline_peaks(shape):
    def inputs(seed):
        return img(shape, seed)

    def call1(f, x, o1):
        f.pipeline(x, out=o1)

    def call2(f, o2):
        f.orientation_peaks(n_angles=16, max_peaks=2, out=(o2[0][0], o2[0][1], o2[1]))
    return inputs, (lambda sec: [sec.out(shape) for _ in range(8)]), (lambda sec: [sec.out((2, 2) + shape), sec.out(shape, np.uint8)]), call1, call2


def _d_batch_nonmax(shape):
    maps = []

    def inputs(seed):
        return np.stack([img(shape, seed + 10 * i) for i in range(3)])

    def call1(f, x, o1):
        f.pipeline_batch(x, out=o1[0])
        f.select_frame(1)

    def call2(f, o2):
        if not maps:
            maps.extend(ready(H.make_map(shape, 40 + k)) for k in range(3))   # (ready long before: made on the first, quiet, use)
        f.nonmax(maps, out=o2)
    return inputs, (lambda sec: [sec.out((3, 8) + shape)]), (lambda sec: [sec.out(shape) for _ in range(3)]), call1, call2


D_PAIRS = {"setup+steer_bank": _d_setup_bank, "pipeline+orientation_peaks": _d_pipeline_peaks, "pipeline_batch+select_frame+nonmax": _d_batch_nonmax}


@pytest.mark.parametrize("first_on_s2", [False, True], ids=["warm_on_s1", "first_call_on_s2"])
@pytest.mark.parametrize("kind,shape", [(2, SMALL), (4, LARGE)])
@pytest.mark.parametrize("pair", sorted(D_PAIRS))
def test_d_stream_hops(pair, kind, shape, first_on_s2):
    """(D) call 1 on a gated stream, call 2 -- which reads only handle state -- on an idle stream right behind it: cvs_set_stream orders the
    new stream behind the old one.  Only the second stream is synchronised.  Then back, with the gate on the other stream."""
    inputs, outs1, outs2, call1, call2 = D_PAIRS[pair](shape)
    s1, s2 = S(0), S(1)
    name = "D %s G%d %dx%d" % (pair, kind, shape[0], shape[1])

    def twin(seed):
        with torch.cuda.stream(s1):
            tw = mk(kind)
            q = G.Section(s1, mode="quiet")
            x, o1, o2 = q.inp(inputs(seed)), outs1(q), outs2(q)
            q.start()
            call1(tw, x, o1)
            s1.synchronize()
            call2(tw, o2)
            s1.synchronize()
            want = [to_np(o) for o in o2]
            close(tw)
        return want

    wants = {seed: twin(seed) for seed in (1, 3)}
    f = mk(kind)
    first = s2 if first_on_s2 else s1
    with torch.cuda.stream(first):   # the handle's first-ever call: on S2 its cvs_set_stream finds a handle that has queued nothing yet
        q = G.Section(first, mode="quiet")
        x, o1, o2 = q.inp(inputs(9)), outs1(q), outs2(q)
        q.start()
        call1(f, x, o1)
        call2(f, o2)
        first.synchronize()
    for a, b, seed in ((s1, s2, 1), (s2, s1, 3)):
        sec = G.behind(a, name=name)
        x, o1, o2 = sec.inp(inputs(seed)), outs1(sec), outs2(sec)
        sec.start()
        with torch.cuda.stream(a):
            call1(f, x, o1)
        with torch.cuda.stream(b):
            call2(f, o2)
        sec.premise("hop to the idle stream")
        b.synchronize()   # only the stream of call 2
        with torch.cuda.stream(b):
            got = [to_np(o) for o in o2]
        check("%s, call 2 after the hop (gate seed %d)" % (name, seed), got, wants[seed])
        a.synchronize()
    close(f)


# ================================================================ E: pool hand-over with work pending
def _release_pool():
    torch.cuda.synchronize()
    L.lib().cvs_release_cached_memory()


@pytest.mark.parametrize("kind,shape", [(2, SMALL), (4, LARGE)])
def test_e_parked_block_is_taken_over_with_its_owner_pending(kind, shape):
    """(E) h1 queues a full setup behind a gate on S1 and is destroyed (no drain: the block is parked with an event); h2 on S2 takes the
    SAME block for another image of the same geometry; only S2 is synchronised"""
    s1, s2 = S(0), S(1)
    with torch.cuda.stream(s2):
        tw = mk(kind)
        tw.setup(ready(img(shape, 2)), FULL)
        s2.synchronize()
        want = snap(tw)
        close(tw)
    _release_pool()
    xb = ready(img(shape, 2))
    with torch.cuda.stream(s1):
        h1 = mk(kind)
        h1.setup(ready(img(shape, 7)), FULL)   # (its block exists before the gate)
        sec = G.behind(s1, name="E hand-over G%d" % kind)
        x = sec.inp(img(shape, 1))
        sec.start()
        h1.setup(x, FULL)
        p1 = h1.basis_view(0)[0]
        close(h1)
        sec.premise("cvs_destroy of a handle without scratch")
    with torch.cuda.stream(s2):
        h2 = mk(kind)
        h2.setup(xb, FULL)
        p2 = h2.basis_view(0)[0]
        assert p2 == p1, "h2 did not take over the block h1 parked"
        sec.premise("the taker's setup")
        s2.synchronize()
        got = snap(h2)
    check_state("E hand-over G%d" % kind, got, want)
    s1.synchronize()   # h1's queue has drained: had h2 not waited for it, h1's setup would have landed on h2's planes only now
    with torch.cuda.stream(s2):
        check_state("E hand-over G%d, after the previous owner's queue has drained" % kind, snap(h2), want)
    close(h2)


@pytest.mark.parametrize("launches", [1, 2])
def test_e_tile_queue_slot_travels_with_its_owner_pending(launches):
    """(E) the same at 1100 x 1500 in the dynamic launch order: the queue slot travels with the block, an odd and an even number of
    launches of the previous owner still pending (cf. test_a_recycled_tile_queue_slot_is_reset_before_its_first_dynamic_launch)"""
    shape, s1, s2 = (1100, 1500), S(0), S(1)
    with torch.cuda.stream(s2):
        tw = mk(2)
        tw.set_option(L.OPT_BLOCK_ORDER, L.ORDER_PLAIN)
        want = [to_np(o) for o in tw.pipeline(ready(img(shape, 2)))]
        wstate = snap(tw)
        close(tw)
    _release_pool()
    xb = ready(img(shape, 2))
    o2 = [torch.full(shape, G.SENTINEL_F32, device=DEV) for _ in range(8)]
    with torch.cuda.stream(s1):
        h1 = mk(2)
        h1.set_option(L.OPT_BLOCK_ORDER, L.ORDER_DYNAMIC_TAIL)
        sec = G.behind(s1, name="E queue slot, %d launches" % launches)
        x, o1 = sec.inp(img(shape, 1)), [sec.out(shape) for _ in range(8)]
        h1.pipeline(ready(img(shape, 7)), out=o1)
        sec.start()
        for _ in range(launches):
            h1.pipeline(x, out=o1)
        p1 = h1.basis_view(0)[0]
        close(h1)
        sec.premise("cvs_destroy")
    with torch.cuda.stream(s2):
        h2 = mk(2)
        h2.set_option(L.OPT_BLOCK_ORDER, L.ORDER_DYNAMIC_TAIL)
        h2.pipeline(xb, out=o2)
        assert h2.basis_view(0)[0] == p1
        s2.synchronize()
        got = [to_np(o) for o in o2]
        gstate = snap(h2)
    check("E queue slot, %d launches" % launches, got, want)
    check_state("E queue slot, %d launches" % launches, gstate, wstate)
    s1.synchronize()
    with torch.cuda.stream(s2):
        check_state("E queue slot, %d launches, after the previous owner's queue has drained" % launches, snap(h2), wstate)
    close(h2)


@pytest.mark.parametrize("variant", ["second_handle_takes_it", "release_cached_memory"])
def test_e_a_handle_that_grows_parks_its_own_block_behind_the_gate(variant):
    """(E) one handle alternates between two geometries behind one gate: growing parks its own block with the small image's launch still
    pending.  Then either a second handle on another stream takes that block, or cvs_release_cached_memory() frees it (it must wait for
    the owner).  The caller-owned pipeline outputs of the owner equal the twin's."""
    s1, s2 = S(0), S(1)
    seq = [(SMALL, 1), (LARGE, 2), (SMALL, 3), (LARGE, 4)]
    with torch.cuda.stream(s1):
        want = []
        for shape, seed in seq + [(SMALL, 5)]:
            tw = mk(2)
            want.append([to_np(o) for o in tw.pipeline(ready(img(shape, seed)))])
            want_state5 = snap(tw)   # (of the last one: image 5)
            close(tw)
    _release_pool()
    x5 = ready(img(SMALL, 5))
    o5 = [torch.full(SMALL, G.SENTINEL_F32, device=DEV) for _ in range(8)]
    with torch.cuda.stream(s1):
        f = mk(2)
        f.pipeline(ready(img(SMALL, 9)))   # the small block exists
        sec = G.behind(s1, name="E own block, " + variant)
        xs = [sec.inp(img(shape, seed)) for shape, seed in seq]
        outs = [[sec.out(shape) for _ in range(8)] for shape, _ in seq]
        sec.start()
        f.pipeline(xs[0], out=outs[0])
        f.pipeline(xs[1], out=outs[1])   # grows: the small block is parked, its launch pending
    if variant == "release_cached_memory":
        L.lib().cvs_release_cached_memory()   # (may wait for the owner; must not free under its launch)
    else:
        with torch.cuda.stream(s2):
            g = mk(2)
            g.pipeline(x5, out=o5)
    with torch.cuda.stream(s1):
        f.pipeline(xs[2], out=outs[2])
        f.pipeline(xs[3], out=outs[3])
        sec.finish()
        for k in range(4):
            check("E own block, %s, call %d" % (variant, k), [to_np(o) for o in outs[k]], want[k])
        close(f)
    if variant != "release_cached_memory":
        with torch.cuda.stream(s2):
            s2.synchronize()
            check("E own block, the taker", [to_np(o) for o in o5], want[4])
            check_state("E own block, the taker's state after the owner's queue has drained", snap(g), want_state5)
            close(g)


# ================================================================ F: scratch growth under load
def test_f_scratch_growth_under_load():
    """(F) a link at 70 x 129 and, behind it in the same gated queue, one at 185 x 256 that grows the component scratch (sync, then free):
    both equal their twins.  Values only: the growth may wait."""
    s = S(0)
    with torch.cuda.stream(s):
        want = []
        for shape, seed in ((SMALL, 1), (LARGE, 2)):
            tw = mk(2)
            tw.setup(ready(img(shape, seed)), BASIS)
            want.append(to_np(tw.link(ready(H.make_map((3,) + shape, seed)), LOW, HIGH, min_area=2)))
            close(tw)
        f = mk(2)
        f.setup(ready(img(SMALL, 9)), BASIS)
        f.link(ready(H.make_map((3,) + SMALL, 9)), LOW, HIGH, min_area=2)
        sec = G.behind(s, name="F scratch growth")
        ms, ml = sec.inp(H.make_map((3,) + SMALL, 1)), sec.inp(H.make_map((3,) + LARGE, 2))
        xl = sec.inp(img(LARGE, 2))
        os_, ol = sec.out((3,) + SMALL, np.uint8), sec.out((3,) + LARGE, np.uint8)
        sec.start()
        f.link(ms, LOW, HIGH, min_area=2, out=os_)
        f.setup(xl, BASIS)
        f.link(ml, LOW, HIGH, min_area=2, out=ol)
        sec.finish()
        check("F scratch growth", [to_np(os_), to_np(ol)], want)
        close(f)


# ================================================================ G: the tuner on a deep queue
def test_g_tuner_on_a_deep_queue():
    """(G) 40 pipeline calls on rotating inputs behind two consecutive gates, no sync, autotune on, on two handles on two streams at once
    (they share the tuner's memory): every one of the 8 outputs of every call equals the CVS_OPT_AUTOTUNE = 0 twin's, the tuner was at work
    on these calls (tune_state 1 = comparing on the caller's launches, or 2 = decided) and launched nothing of its own"""
    shape, n, rot = (1024, 1040), 40, 4
    streams = [S(0), S(1)]
    with torch.cuda.stream(streams[0]):
        tw = mk(2)
        tw.set_option(L.OPT_AUTOTUNE, 0)
        want = []
        for i in range(rot):
            o = torch.empty((8,) + shape, device=DEV)
            tw.pipeline(ready(img(shape, i)), out=list(o))
            streams[0].synchronize()
            want.append(o)
        assert tw.launch_info()["tune_state"] == 0
        close(tw)
    hs, secs, xs, outs = [], [], [], []
    for s in streams:
        with torch.cuda.stream(s):
            f = mk(2)
            f.set_option(L.OPT_AUTOTUNE, 1)
            f.pipeline(ready(img(shape, 9)))   # state exists
            hs.append(f)
            sec = G.behind(s, name="G tuner")
            xs.append([sec.inp(img(shape, i)) for i in range(rot)])
            outs.append([torch.full((8,) + shape, G.SENTINEL_F32, device=DEV) for _ in range(n)])   # (sentinel made on the device: 2.7 GB)
            secs.append(sec)
    for k, sec in enumerate(secs):
        sec.start(sync=k == 0)   # (the second section's device sync would wait the first one's gate out)
        sec.regate()             # two consecutive gates
    for i in range(n):
        for k, s in enumerate(streams):
            with torch.cuda.stream(s):
                hs[k].pipeline(xs[k][i % rot], out=list(outs[k][i]))
    for k, s in enumerate(streams):
        with torch.cuda.stream(s):
            secs[k].finish()
            info = hs[k].launch_info()
            assert info["tune_state"] >= 1 and info["tuning_launches"] == 0, info
            for i in range(n):
                for j in range(8):
                    assert torch.equal(outs[k][i][j].view(torch.int32), want[i % rot][j].view(torch.int32)), "G tuner: handle %d, call %d, output %d differs from the autotune-off twin" % (k, i, j)
            close(hs[k])


# ================================================================ H: the Python batch layer
def test_h_native_batch_waits_for_the_callers_stream():
    """(H) NativeBatch.run works on streams of its own: frames that get their values late on torch's current stream must have landed
    before it starts (the synchronize() of batch.py)"""
    shape, n, s = (70, 200), 5, S(0)
    frames = np.stack([img(shape, i) for i in range(n)])
    with torch.cuda.stream(s):
        tw = mk(2)
        want = to_np(tw.pipeline_batch(ready(frames), outputs=(5, 6, 7)))
        close(tw)
        nb = batch.NativeBatch.local((0,))
        nb.run(ready(frames[::-1].copy()), n, shape, outputs=(5, 6, 7))   # staging exists
        sec = G.behind(s, name="H batch layer")
        fr, out = sec.inp(frames), sec.out((n, 3) + shape)
        sec.start()
        got, _ = nb.run(fr, n, shape, outputs=(5, 6, 7), out=out)
        got = to_np(got)
        sec.finish()
        nb.close()
    check("H batch layer", [got], [want])
