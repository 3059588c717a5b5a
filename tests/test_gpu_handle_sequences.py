"""GPU test (-m gpu): ONE long-lived handle walked through a history, against fresh handles (tests/handle_sequences.py).

The committed seeds of handle_sequences.COMMITTED run against the real engine through cvsteer_amd/api.py (raw C ABI calls where the
Python surface has no method: cvs_setup_rows, cvs_num_frames).  After every step the long-lived handle's state planes and one read-only
call are compared bit for bit with a fresh handle brought to the same state by one call; statuses come from the contract model; the
last observation of every sequence is also held to the float64 oracle at the suite's 1e-5.  The directed histories (a) .. (i) are
hand-written sequences under the same rule.  No comparison is masked or skipped (the runner's 'skipped' counter is asserted 0).

Wall time per case on an MI355X (pytest --durations, one run of this module, 27 cases in 4.5 s with start-up):
  committed G2 seeds 0 .. 11:  0.40 (the first case: it also loads the library and warms the device), 0.10, 0.09, 0.10, 0.11, 0.11, 0.07,
                               0.09, 0.09, 0.10, 0.09, 0.08 s
  committed G4 seeds 0 .. 5:   0.14, 0.14, 0.08, 0.11, 0.10, 0.09 s
  directed (a) .. (i):         0.04, 0.10, 0.03, 0.04, 0.17, 0.05, 0.04, 0.03, 0.03 s
A sequence of 60 steps builds 28 .. 75 fresh twins and compares 0.2 .. 6 million values; nothing needed trimming.
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import cvsteer_amd as cv
import handle_sequences as H
from cvsteer_amd import _lib as L
from handle_sequences import BASIS, FULL, OK, Op

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5   # test_g2_basis_matches_oracle / test_g4_basis_matches_oracle

STATUS = {0: OK, -1: H.E_BADARG, -2: H.E_SIZE, -5: H.E_STATE, -6: H.E_UNSUPPORTED}
OPTIONS = {"atan": L.OPT_ATAN_MODE, "strip": L.OPT_STRIP_ROWS, "find_on": L.OPT_FIND_ON, "order": L.OPT_BLOCK_ORDER,
           "persist": L.OPT_PERSIST_STATE, "layout": L.OPT_STATE_LAYOUT, "autotune": L.OPT_AUTOTUNE, "overlap": L.OPT_HOST_OVERLAP,
           "g4_ext": L.OPT_G4_EXTENSIONS}
_STREAMS = []
_HIP_ERROR = []   # set by the first HIP error: the session ends, nothing further is started on the device


def _stream(idx):
    while len(_STREAMS) < 2:
        _STREAMS.append(torch.cuda.Stream(DEV))
    return _STREAMS[idx]


def _np(x):
    if torch.is_tensor(x):
        return x.cpu().numpy()
    if isinstance(x, np.ndarray) and x.dtype.names:   # record arrays (chain measures): their bytes
        return np.frombuffer(x.tobytes(), np.uint8)
    return np.asarray(x)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _View:
    """a device plane by address, for torch.as_tensor"""

    def __init__(self, ptr, rows, cols, step):
        self.__cuda_array_interface__ = {"shape": (rows, cols), "strides": (step, 4), "typestr": "<f4", "data": (ptr, False), "version": 2}


class Engine:
    """the handle_sequences engine over cvsteer_amd.api"""

    def __init__(self, kind):
        self.kind, self.nb = kind, H.NB[kind]
        if kind == 2:
            self.f = cv.SteerableFiltersG2(None)
        else:
            # (the Python object is told extensions=True so that it forwards every call; whether the ENGINE has them on is the
            # sequence's CVS_OPT_G4_EXTENSIONS, off on a fresh handle as in the C ABI)
            self.f = cv.SteerableFiltersG4(None, extensions=True)
            self.f.set_option(L.OPT_G4_EXTENSIONS, 0)
        self.si = None

    def close(self):
        f, self.f = self.f, None
        if f is not None:
            f.__del__()

    def apply(self, op):
        ctx = torch.cuda.stream(_stream(self.si)) if self.si is not None else torch.cuda.stream(torch.cuda.default_stream(DEV))
        try:
            with ctx:
                res = getattr(self, "op_" + op.name)(op)
                return OK, tuple(_np(r) for r in res)
        except cv.CvsError as e:
            if e.status not in STATUS:
                _HIP_ERROR.append(str(e))
            return STATUS.get(e.status, H.E_HIP), None
        except RuntimeError as e:   # a HIP error surfacing through torch: nothing further is issued
            _HIP_ERROR.append("%r: %s" % (op, e))
            return H.E_HIP, None

    def state(self):
        out = []
        for p in range(self.nb + 5):
            st, res = self.apply(Op("read_state", which=p))
            out.append((st, res[0] if res else None))
        return out

    def _raw(self, rc, where):
        if rc:
            raise cv.CvsError(rc, where)

    def _image(self, img, host=False):
        a = H.make_image(img)
        return a if host else _dev(a)

    # -- state-establishing calls
    def op_setup(self, op):
        self.f.setup(self._image(op.img), op.flags)
        return ()

    def op_setup_steer(self, op):
        t = self._image(op.img)
        out = None
        if op.get("bad") == "size":
            out = [torch.empty((t.shape[0] + 1, t.shape[1]), dtype=torch.float32, device=DEV) for _ in range(2)]
        elif op.get("bad") == "overlap":
            out = [t, torch.empty_like(t)]
        return self.f.setup_steer(t, op.theta, op.flags, out=out)

    def op_setup_pyr(self, op):
        return (self.f.setup_pyr(self._image(op.img), op.flags),)

    def op_setup_rows(self, op):
        t = self._image(op.img)
        f = self.f
        f._like = f._image_keepalive = t
        f._bind_stream(t)
        p = cv.api._plane(t)
        self._raw(L.lib().cvs_setup_rows(f._h, C.byref(p), op.flags, op.lo, op.hi), "cvs_setup_rows")
        return ()

    def op_pipeline(self, op):
        img = self._image(op.img, op.host)
        rows, cols = img.shape
        outs = [None] * 8
        for k in op.subset:
            if op.host:
                outs[k] = np.empty((rows, cols), np.uint8 if op.u8out else np.float32)
            else:
                outs[k] = torch.empty((rows, cols), dtype=torch.uint8 if op.u8out else torch.float32, device=DEV)
        if op.get("bad") == "size":
            outs[op.subset[0]] = torch.empty((rows, cols + 1), dtype=torch.float32, device=DEV)
        elif op.get("bad") == "overlap":
            outs[op.subset[0]] = img
        self.f.pipeline(img, out=outs)
        return [outs[k] for k in op.subset]

    def _frames(self, imgs, scattered):
        arrs = [H.make_image(i) for i in imgs]
        if not scattered:
            return _dev(np.stack(arrs))
        frames = []
        for i, a in enumerate(arrs):   # separate allocations with two row pitches: no constant stride, no common step
            t = torch.empty((a.shape[0], a.shape[1] + 4 * (i % 2) + 4), dtype=torch.from_numpy(a).dtype, device=DEV)[:, :a.shape[1]]
            t.copy_(torch.from_numpy(a))
            frames.append(t)
        return frames

    def op_pipeline_batch(self, op):
        rows, cols = op.imgs[0][:2]
        dt = torch.uint8 if op.u8out else torch.float32
        if op.get("bad") == "size":
            frames = self._frames(op.imgs, True)
            out = torch.empty((len(frames), len(op.subset), rows + 1, cols), dtype=dt, device=DEV)
            return (self.f.pipeline_batch(frames, out=out, outputs=op.subset),)
        return (self.f.pipeline_batch(self._frames(op.imgs, op.scattered), outputs=op.subset, dtype=dt),)

    def op_contours_batch(self, op):
        return (self.f.contours_batch(self._frames(op.imgs, False), H.LOW, H.HIGH),)

    def op_contour_edgels_batch(self, op):
        return self.f.contour_edgels_batch(self._frames(op.imgs, False), H.LOW, H.HIGH)

    # -- frames and state reads
    def op_select_frame(self, op):
        self.f.select_frame(op.i)
        return ()

    def op_num_frames(self, op):
        n = C.c_int(-1)
        self._raw(L.lib().cvs_num_frames(self.f._h, C.byref(n)), "cvs_num_frames")
        return (np.int64(n.value),)

    def op_shape(self, op):
        return (np.array(self.f.shape, np.int64),)

    def _code(self, p):
        return L.PLANE_BASIS0 + p if p < self.nb else L.PLANE_C1 + (p - self.nb)

    def op_read_state(self, op):
        return (self.f._state(self._code(op.which)),)

    def op_coefficients(self, op):
        return self.f.coefficients()

    def op_basis_view(self, op):
        ptr, rows, cols, step = self.f.basis_view(op.p)
        self.f.sync()
        plane = torch.as_tensor(_View(ptr, rows, cols, step), device=DEV).clone()
        return (np.array((rows, cols), np.int64), plane)

    # -- read-only calls
    def _bad_outs(self, n):
        rows, cols = self.f.shape
        return [torch.empty((rows + 1, cols), dtype=torch.float32, device=DEV) for _ in range(n)]

    def op_steer_scalar(self, op):
        return self.f.steer(op.theta, op.full, out=self._bad_outs(5 if op.full else 2) if op.get("bad") == "size" else None)

    def op_steer_map(self, op):
        return self.f.steer(None, op.full, out=self._bad_outs(5 if op.full else 2) if op.get("bad") == "size" else None)

    def op_steer_bank(self, op):
        return self.f.steer_bank(op.thetas, full=op.full)

    def op_steer_point(self, op):
        return (np.array(cv.SteerableFiltersG2.steer_point(self.f, (op.x, op.y), op.theta, full=True), np.float32),)

    def op_nonmax(self, op):
        m = _dev(H.make_map(tuple(op.shape), op.seed))
        return (self.f.nonmax(m, out=m if op.get("bad") == "overlap" else None),)

    def op_chain_refine(self, op):
        shape = tuple(op.shape)
        return self.f.chain_refine(_dev(H.make_points(shape, op.seed)), _dev(H.make_map(shape, op.seed)))

    # -- the contour tail
    def op_hysteresis(self, op):
        return (self.f.hysteresis(_dev(H.make_map(tuple(op.shape), op.seed)), H.LOW, H.HIGH),)

    def op_label(self, op):
        labels, count = self.f.label(_dev(H.make_mask(tuple(op.shape), op.seed, op.dense)))
        return (labels, np.int64(count))

    def op_link(self, op):
        return (self.f.link(_dev(H.make_map(tuple(op.shape), op.seed)), H.LOW, H.HIGH, min_area=2),)

    def op_contour_chains(self, op):
        return self.f.contour_chains(_dev(H.make_mask(tuple(op.shape), op.seed, op.dense)))

    def op_contour_edgels(self, op):
        shape = tuple(op.shape)
        return self.f.contour_edgels(_dev(H.make_mask(shape, op.seed, False)), _dev(H.make_map(shape, op.seed)), theta=_dev(H.make_theta(shape, op.seed)))

    # -- options and streams
    def op_set_option(self, op):
        self.f.set_option(OPTIONS[op.opt], op.value)
        return ()

    def op_set_u8_gain(self, op):
        self.f.set_u8_gain(op.gain)
        return ()

    def op_set_stream(self, op):
        self.si = op.idx
        return ()


@pytest.fixture(scope="module")
def oracle(ora):
    def basis(kind, img):
        w, s = H.TAPS[kind]
        return np.asarray(ora.basis(kind, H.make_image(img), w, s, f64=True), np.float64)
    return basis


def _run(kind, seq, seed, oracle=None):
    if _HIP_ERROR:
        pytest.exit("a HIP error earlier in this session: %s" % _HIP_ERROR[0], returncode=3)
    t0 = time.perf_counter()
    stats = H.run(Engine, kind, seq, seed, oracle=oracle, tol=TOL)
    stats["seconds"] = time.perf_counter() - t0
    print("G%d %s: %s" % (kind, seed, stats))
    assert stats["skipped"] == 0 and stats["steps"] == len(seq) and stats["observations"] > 0
    return stats


@pytest.mark.parametrize("kind,seed", [(k, s) for k in (2, 4) for s in H.COMMITTED[k]])
def test_committed_sequence(kind, seed, oracle):
    stats = _run(kind, H.generate(kind, seed, H.LENGTH), seed, oracle)
    assert stats["oracle_err"] <= TOL


IMG = lambda shape, seed, u8=False: (shape[0], shape[1], seed, u8)
BIG, MID, SMALL = (131, 257), (33, 130), (19, 7)


def test_a_basis_only_setup_drops_the_orientation_of_the_previous_image(oracle):
    """(a) full setup, then a basis-only setup of another image of the same size: every theta-NULL entry and coefficients() answer
    CVS_E_STATE (the runner asks each of them), the basis planes are those of the new image"""
    for kind, ext in ((2, []), (4, [Op("set_option", opt="g4_ext", value=1)])):
        _run(kind, ext + [Op("setup", img=IMG(MID, 1), flags=FULL), Op("setup", img=IMG(MID, 2), flags=BASIS), Op("coefficients"),
                          Op("steer_map", full=False), Op("nonmax", shape=MID, seed=3), Op("chain_refine", shape=MID, seed=3),
                          Op("steer_scalar", theta=0.4, full=True), Op("read_state", which=H.NB[kind] + 3)], "a", oracle)


def test_b_single_setup_after_a_batch_leaves_one_frame():
    """(b) pipeline_batch(5), select_frame(4), a single-image setup: one frame, frame 0 selected, select_frame(4) refused; a
    following pipeline_batch(2) addresses frame 0"""
    five = tuple(IMG(MID, s) for s in range(5))
    _run(2, [Op("pipeline_batch", imgs=five, scattered=False, u8out=False, subset=(0, 1, 5)), Op("select_frame", i=4),
             Op("setup", img=IMG(MID, 9), flags=FULL), Op("num_frames"), Op("select_frame", i=4), Op("select_frame", i=1),
             Op("pipeline_batch", imgs=five[:2], scattered=True, u8out=False, subset=(2,)), Op("num_frames"), Op("select_frame", i=1),
             Op("select_frame", i=2), Op("pipeline_batch", imgs=five, scattered=True, u8out=False, subset=(5, 6, 7)), Op("select_frame", i=3),
             Op("pipeline_batch", imgs=five[3:], scattered=False, u8out=False, subset=(7,))], "b")


def test_c_three_geometries_large_small_large():
    """(c) the state block re-laid for 320-, 64- and 192-column pitches, large / small / large: equal to the twin each time"""
    order = [BIG, SMALL, BIG, MID, SMALL, MID, BIG]
    _run(2, [Op("setup", img=IMG(s, i), flags=FULL if i % 2 else BASIS) for i, s in enumerate(order)], "c")
    _run(4, [Op("setup", img=IMG(s, i), flags=BASIS) for i, s in enumerate(order)], "c")
    e, pitches = Engine(2), set()
    for i, s in enumerate(order):
        assert e.apply(Op("setup", img=IMG(s, i), flags=BASIS))[0] == OK
        step = e.f.basis_view(0)[3]
        pitch = (s[1] + 63) // 64 * 64
        assert step % (4 * pitch) == 0 and step // (4 * pitch) in (1, 7, 12)
        pitches.add(pitch)
    e.close()
    assert pitches == {64, 192, 320}


def test_d_outputs_only_pipeline_leaves_no_state_addressable():
    """(d) a full setup of image A, then a pipeline on image B with CVS_OPT_PERSIST_STATE = 0: every state-reading entry answers
    CVS_E_STATE (the runner asks each), cvs_shape is (0, 0), cvs_num_frames 0 -- A's planes are not addressable"""
    for kind, ext in ((2, []), (4, [Op("set_option", opt="g4_ext", value=1)])):
        for shape_b in (MID, SMALL):
            _run(kind, ext + [Op("setup", img=IMG(MID, 1), flags=FULL), Op("set_option", opt="persist", value=0),
                              Op("pipeline", img=IMG(shape_b, 2), u8out=False, subset=(0, 5), host=False), Op("shape"), Op("num_frames"),
                              Op("read_state", which=0), Op("pipeline", img=IMG(shape_b, 3), u8out=True, subset=(5, 6, 7), host=False),
                              Op("pipeline_batch", imgs=(IMG(shape_b, 4), IMG(shape_b, 5)), scattered=False, u8out=False, subset=(5,)),
                              Op("read_state", which=0), Op("select_frame", i=2)], "d")


def test_e_band_after_a_whole_image_setup():
    """(e) cvs_setup_rows behind a whole-image setup with the same flags: inside the band the planes of the new image, outside the
    earlier bits (the runner stitches the two twins row by row).  With OTHER flags the header's rule holds: the band's rows are those of
    the new image, orientation state follows the band's flags, and the rows outside the band are unspecified (not compared)."""
    shape = (70, 129)
    for kind, flags in ((2, FULL), (2, BASIS), (4, BASIS)):
        for layout in (1, 0, 3):
            _run(kind, [Op("set_option", opt="layout", value=layout), Op("setup", img=IMG(shape, 1), flags=flags),
                        Op("setup_rows", img=IMG(shape, 2), flags=flags, lo=20, hi=45), Op("steer_scalar", theta=0.3, full=False),
                        Op("setup_rows", img=IMG(shape, 3, True), flags=flags, lo=40, hi=70), Op("steer_bank", thetas=[0.2, 1.1], full=False),
                        Op("setup_rows", img=IMG(shape, 4), flags=flags, lo=0, hi=1)], "e")
    for first, band in ((FULL, BASIS), (BASIS, FULL)):
        e, tw = Engine(2), Engine(2)
        assert e.apply(Op("setup", img=IMG(shape, 1), flags=first))[0] == OK
        assert e.apply(Op("setup_rows", img=IMG(shape, 2), flags=band, lo=20, hi=45))[0] == OK
        assert tw.apply(Op("setup", img=IMG(shape, 2), flags=band))[0] == OK
        got, want = e.state(), tw.state()
        for p in range(12):
            assert got[p][0] == want[p][0] == (OK if (p < 7 or band == FULL) else H.E_STATE), p
            if got[p][0] == OK:
                assert np.array_equal(got[p][1][20:45].view(np.uint32), want[p][1][20:45].view(np.uint32)), p
        e.close()
        tw.close()


def test_f_contour_tail_small_large_small():
    """(f) the contour tail's scratch blocks grow, stay and are reused: labels, point lists, chains and refined points on a small
    image, a large one and the small one again, each equal to a fresh handle's; the dense mask behind a sparse one of the same size makes
    the arc arrays grow in a call whose planes already live in the component scratch"""
    seq = []
    for i, s in enumerate((SMALL, BIG, SMALL, MID)):
        seq.append(Op("setup", img=IMG(s, i), flags=FULL))
        seq += [Op("contour_chains", shape=s, seed=i, dense=False), Op("contour_chains", shape=s, seed=i, dense=True),
                Op("label", shape=s, seed=i, dense=True), Op("hysteresis", shape=s, seed=i), Op("link", shape=s, seed=i),
                Op("contour_edgels", shape=s, seed=i), Op("chain_refine", shape=s, seed=i), Op("nonmax", shape=s, seed=i),
                Op("contour_chains", shape=BIG if s != BIG else MID, seed=i, dense=False)]
    seq += [Op("contours_batch", imgs=(IMG(MID, 1), IMG(MID, 2))), Op("contour_edgels_batch", imgs=(IMG(SMALL, 1), IMG(SMALL, 2), IMG(SMALL, 3))),
            Op("select_frame", i=2), Op("contours_batch", imgs=(IMG(BIG, 1),))]
    _run(2, seq, "f")
    # the sizing calls of the Python surface answer CVS_E_SIZE for "more than capacity"; a plane of another size must not pass for that
    e = Engine(2)
    assert e.apply(Op("setup", img=IMG(SMALL, 1), flags=BASIS))[0] == OK
    for call in (lambda: e.f.contour_chains(torch.zeros(MID, dtype=torch.uint8, device=DEV)),
                 lambda: e.f.contour_chains(np.zeros(MID, np.uint8)),
                 lambda: e.f.contour_points(torch.zeros(MID, dtype=torch.int32, device=DEV)),
                 lambda: e.f.contour_chains_batch(torch.zeros((2,) + MID, dtype=torch.uint8, device=DEV))):
        with pytest.raises(cv.CvsError) as err:
            call()
        assert err.value.status == L.E_SIZE
    pts, chains = e.f.contour_chains(torch.zeros(SMALL, dtype=torch.uint8, device=DEV))   # an empty mask is no error
    assert tuple(pts.shape) == (0, 2) and tuple(chains.shape) == (0, 4)
    e.close()


def test_g_u8_gain_changes_between_pipeline_calls():
    """(g) the u8 gain changed between two pipeline calls, the u8 scratch growing from the small image to the large one"""
    pipe = lambda s, seed, subset: Op("pipeline", img=IMG(s, seed), u8out=True, subset=subset, host=False)
    seq = [pipe(SMALL, 1, (5, 6, 7)), Op("set_u8_gain", gain=3.0), pipe(SMALL, 1, (5, 6, 7)), pipe(BIG, 2, (0, 3, 5)),
           Op("set_u8_gain", gain=0.0), pipe(BIG, 2, (0, 3, 5)), Op("set_option", opt="persist", value=0), pipe(MID, 3, (5, 6, 7)),
           Op("set_u8_gain", gain=0.5), pipe(BIG, 3, (5, 6, 7)), Op("set_option", opt="persist", value=1),
           Op("pipeline_batch", imgs=(IMG(MID, 1), IMG(MID, 2)), scattered=False, u8out=True, subset=(5, 6, 7))]
    _run(2, seq, "g")
    _run(4, [Op("set_option", opt="g4_ext", value=1)] + seq, "g")


def test_h_stream_switch_between_a_setup_and_its_reads():
    """(h) the reads of a setup run on another stream than the setup: the new stream waits for the old one"""
    seq = []
    for i in range(4):
        seq += [Op("set_stream", idx=i % 2), Op("setup", img=IMG(BIG, i), flags=FULL), Op("set_stream", idx=(i + 1) % 2),
                Op("steer_map", full=True), Op("read_state", which=3)]
    _run(2, seq, "h")


def test_i_two_handles_on_two_streams_trade_pooled_blocks():
    """(i) destroy and re-create with a second live handle on another stream holding and releasing blocks of the same size: the pool
    hands blocks over with work pending, and every result equals its twin"""
    seq = []
    for i in range(4):
        seq += [Op("set_stream", idx=i % 2), Op("setup", img=IMG(BIG, i), flags=FULL), Op("recreate", shape=BIG),
                Op("pipeline_batch", imgs=(IMG(BIG, 10 + i), IMG(BIG, 20 + i)), scattered=False, u8out=False, subset=(0,)), Op("recreate", shape=BIG)]
    _run(2, seq, "i")
    # the same by hand: two live handles, blocks released by one are taken by the other while its launches are still queued
    a, b = Engine(2), Engine(2)
    a.si, b.si = 0, 1
    for i in range(3):
        assert a.apply(Op("setup", img=IMG(BIG, i), flags=FULL))[0] == OK
        a.close()
        assert b.apply(Op("setup", img=IMG(BIG, 50 + i), flags=FULL))[0] == OK   # takes the block `a` parked, its event pending
        a = Engine(2)
        a.si = 0
        tw = Engine(2)
        assert tw.apply(Op("setup", img=IMG(BIG, 50 + i), flags=FULL))[0] == OK
        for (s0, p0), (s1, p1) in zip(b.state(), tw.state()):
            assert s0 == s1 == OK and np.array_equal(p0.view(np.uint32), p1.view(np.uint32))
        tw.close()
        b.close()
        b = Engine(2)
        b.si = 1
    a.close()
    b.close()
