"""Long-lived handles against fresh ones over random call sequences (test infrastructure; engine-agnostic: it never imports the engine).

Three parts:
  * Model -- the CONTRACT of a handle as include/cvsteer_hip.h states it: kind, options, u8 gain, image shape, have_basis / have_orient,
    frames and the selected frame, and for every frame WHICH input and WHICH state-establishing call its state came from (for
    cvs_setup_rows: which row range came from which call).  For every operation it answers the expected status and the RECIPE of the
    expected values: the shortest call list that establishes the same state on a fresh handle (options as they were, one
    state-establishing call, options as they are, select_frame), after which the observation is repeated on that twin.
  * generate(kind, seed, length) -- a seeded generator of call sequences over the whole operation alphabet.
  * run(engine_factory, kind, sequence) -- drives ONE engine through the sequence; after every step that may change state (refused calls
    included) it compares every state plane of the selected frame plus one generated read-only call, bit for bit, with the twin; where
    the model says state is missing it asks every state-reading entry for the model's status.  Nothing is masked, nothing is skipped.

An engine is any object with
    apply(op) -> (status, result)   status one of the strings below, result a tuple of numpy arrays (None when refused)
    state()   -> [(status, array or None)] for the nb + 5 state planes of the selected frame
    close()
Two exist: the numpy surrogate of test_handle_sequences_cpu.py (with injectable faults) and the adapter of
test_gpu_handle_sequences.py over cvsteer_amd/api.py.

Rules the model takes from the header, spelled out because sequences lean on them:
  * a refused call changes nothing; refusals used here are the ones the argument checks make before anything is queued;
  * cvs_shape / cvs_num_frames report (0, 0) / 0 without state; the contour tail keeps the image size of the last state-establishing
    call, kept state or not (CVS_E_STATE only "before the first setup");
  * cvs_select_frame(i) is valid for 0 <= i < n of the last state-establishing call (1 for single images and fresh handles);
  * cvs_setup_rows: outside the band the rows keep their bits when the previous state-establishing call was a cvs_setup /
    cvs_setup_steer / cvs_setup_pyr / cvs_setup_rows of an image of the same size with the same flags and CVS_OPT_STATE_LAYOUT value
    (sequences issue bands only then); images that take the generic path are filtered whole.
"""
import random
import zlib

import numpy as np

OK, E_BADARG, E_SIZE, E_STATE, E_UNSUPPORTED, E_HIP = "OK", "E_BADARG", "E_SIZE", "E_STATE", "E_UNSUPPORTED", "E_HIP"
BASIS, FULL = 1, 3
NB = {2: 7, 4: 11}
TAPS = {2: (4, 0.67), 4: (6, 0.5)}
# straddle rows >= 3W+1 / cols >= W+1 of the fast paths (W = 4: 13 x 5, W = 6: 19 x 7) and the 64-column strips
SHAPES = [(1, 1), (7, 1), (12, 70), (13, 5), (18, 7), (19, 7), (19, 65), (33, 130), (70, 129), (131, 257)]
OPTION_VALUES = {"atan": (0, 1), "strip": (0, 3, 8), "find_on": (0, 1), "order": (0, 1000000, 2000000), "persist": (0, 1),
                 "layout": (0, 1, 2, 3), "autotune": (0, 1), "overlap": (0, 1), "g4_ext": (0, 1)}
OPTION_DEFAULTS = {"atan": 0, "strip": 0, "find_on": 0, "order": -1, "persist": 1, "layout": 1, "autotune": 1, "overlap": 1, "g4_ext": 0}
GAINS = (0.0, 1.0, 0.5, 3.0)
ESTABLISHING = ("setup", "setup_steer", "setup_pyr", "setup_rows", "pipeline", "pipeline_batch")
TAIL_ESTABLISHING = ("contours_batch", "contour_edgels_batch")
STATE_READS = ("select_frame", "num_frames", "shape", "read_state", "coefficients", "basis_view")
READ_ONLY = ("steer_scalar", "steer_map", "steer_bank", "steer_point", "nonmax", "chain_refine")
TAIL = ("hysteresis", "label", "link", "contour_chains", "contour_edgels") + TAIL_ESTABLISHING
OTHER = ("set_option", "set_u8_gain", "set_stream", "recreate")
KINDS = ESTABLISHING + STATE_READS + READ_ONLY + TAIL + OTHER
LOW, HIGH = 0.55, 0.8   # thresholds of every contour call (maps are uniform on [0, 1))
# the committed sequences: generate(kind, seed, LENGTH) for every seed below (test_handle_sequences_cpu.py holds them to its coverage and
# fault-detection conditions, test_gpu_handle_sequences.py runs them on the engine)
LENGTH = 60
COMMITTED = {2: tuple(range(12)), 4: tuple(range(6))}


class Op:
    """one call: a name and keyword arguments; repr() is Python that rebuilds it (for replaying a reported case by hand)"""
    __slots__ = ("name", "a")

    def __init__(self, name, **a):
        self.name, self.a = name, a

    def __getattr__(self, k):
        try:
            return self.a[k]
        except KeyError:
            raise AttributeError(k)

    def get(self, k, default=None):
        return self.a.get(k, default)

    def __repr__(self):
        return "Op(%r%s)" % (self.name, "".join(", %s=%r" % kv for kv in sorted(self.a.items())))

    def __eq__(self, o):
        return isinstance(o, Op) and repr(self) == repr(o)

    def __hash__(self):
        return hash(repr(self))


# ---------------------------------------------------------------- inputs, shared by every engine (an image is (rows, cols, seed, u8))
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def make_image(img):
    rows, cols, seed, u8 = img
    r = _rng("image", rows, cols, seed)
    return r.integers(0, 256, (rows, cols), dtype=np.uint8) if u8 else r.random((rows, cols), dtype=np.float32)


def make_map(shape, seed):
    """an un-thinned response: uniform on [0, 1)"""
    return _rng("map", shape, seed).random(shape, dtype=np.float32)


def make_theta(shape, seed):
    return ((_rng("theta", shape, seed).random(shape, dtype=np.float32) - np.float32(0.5)) * np.float32(np.pi)).astype(np.float32)


def make_mask(shape, seed, dense):
    """bytes: sparse (a few short arcs) or dense (most pixels set: about four directed links per pixel, the most a mask can have)"""
    return (_rng("mask", shape, seed).random(shape) < (0.85 if dense else 0.08)).astype(np.uint8) * np.uint8(255)


def make_points(shape, seed, n=37):
    r = _rng("points", shape, seed)
    return np.stack([r.integers(0, shape[1], n), r.integers(0, shape[0], n)], axis=1).astype(np.int32)


def generic_path(kind, shape):
    w = TAPS[kind][0]
    return shape[0] < 3 * w + 1 or shape[1] < w + 1


# ---------------------------------------------------------------- the contract model
class Model:
    def __init__(self, kind):
        self.kind, self.nb = kind, NB[kind]
        self.reset()

    def reset(self):
        self.opts = dict(OPTION_DEFAULTS)
        self.gain = 0.0
        self.have_basis = self.have_orient = False
        self.shape = None          # of the state
        self.tail_shape = None     # image size the contour tail works at
        self.slots = 1             # frames of the last state-establishing call
        self.cur = 0
        self.frames = []           # per frame: [(row_lo, row_hi, source)], source = (establishing Op, frame in it, options then)
        self.last_est = None       # (name, flags, shape, layout) of the last state-establishing call

    def options(self):
        return tuple(sorted(self.opts.items())) + (("gain", self.gain),)

    # -- expected status, in the order of the argument checks; sequences break one rule at a time
    def _caller_ok(self):
        return self.kind == 2 or self.opts["g4_ext"] == 1

    def status(self, op):
        n, k4, ext = op.name, self.kind == 4, self.opts["g4_ext"] == 1
        bad = op.get("bad")
        if n in ("setup", "setup_pyr", "setup_steer"):
            if (op.flags & 2) and k4 and not ext:
                return E_UNSUPPORTED
            return {None: OK, "size": E_SIZE, "overlap": E_BADARG}[bad]
        if n == "setup_rows":
            if (op.flags & 2) and k4:
                return E_UNSUPPORTED
            return OK
        if n in ("pipeline", "pipeline_batch"):
            if not self._caller_ok():
                return E_UNSUPPORTED
            return {None: OK, "size": E_SIZE, "overlap": E_BADARG}[bad]
        if n in TAIL_ESTABLISHING:
            if not self._caller_ok():
                return E_UNSUPPORTED
            return OK if self.opts["persist"] else E_STATE
        if n == "select_frame":
            return OK if 0 <= op.i < self.slots else E_BADARG
        if n in ("num_frames", "shape", "set_option", "set_u8_gain", "set_stream", "recreate"):
            return OK
        if n == "read_state":
            return OK if (self.have_orient if op.which >= self.nb else self.have_basis) else E_STATE
        if n == "coefficients":
            return OK if self.have_orient else E_STATE
        if n == "basis_view":
            return OK if self.have_basis else E_STATE
        if n in ("steer_scalar", "steer_map", "steer_bank"):
            if not self.have_basis:
                return E_STATE
            if bad == "size":
                return E_SIZE
            if op.full and k4 and not ext:
                return E_UNSUPPORTED
            if (op.full or n == "steer_map") and not self.have_orient:
                return E_STATE
            return OK
        if n == "steer_point":
            if k4:
                return E_UNSUPPORTED
            return OK if self.have_basis else E_STATE
        if n in ("nonmax", "chain_refine"):
            if not self.have_orient:
                return E_STATE
            if tuple(op.shape) != self.shape:
                return E_SIZE
            return E_BADARG if bad == "overlap" else OK
        if n in ("hysteresis", "label", "link", "contour_chains", "contour_edgels"):
            if self.tail_shape is None:
                return E_STATE
            return OK if tuple(op.shape) == self.tail_shape else E_SIZE
        raise ValueError(n)

    def band_allowed(self, op):
        """the rule of cvs_setup_rows: rows outside the band are defined only after a whole-image setup of that size, flags and layout"""
        return self.have_basis and self.last_est == (True, op.flags | 1, tuple(op.img[:2]), self.opts["layout"]) and self.slots == 1

    # -- state transitions of a call whose status is OK
    def apply(self, op):
        n = op.name
        if n == "set_option":
            self.opts[op.opt] = op.value
        elif n == "set_u8_gain":
            self.gain = op.gain
        elif n == "recreate":
            self.reset()
        elif n == "select_frame":
            self.cur = op.i
        elif n in ESTABLISHING or n in TAIL_ESTABLISHING:
            imgs = op.imgs if n in ("pipeline_batch",) + TAIL_ESTABLISHING else [op.img]
            shape, then = tuple(imgs[0][:2]), self.options()
            if n == "setup_rows":
                if not self.band_allowed(op):
                    raise AssertionError("sequence issues a band where the header leaves the other rows undefined: %r" % (op,))
                src = (Op("setup", img=op.img, flags=op.flags), 0, then)
                if generic_path(self.kind, shape):
                    self.frames = [[(0, shape[0], src)]]
                else:
                    old = [(lo, hi, s) for (lo, hi, s) in self._cut(self.frames[0], op.lo, op.hi)]
                    self.frames = [sorted(old + [(op.lo, op.hi, src)], key=lambda t: t[0])]
                return
            pipe = n not in ("setup", "setup_steer", "setup_pyr")
            flags = FULL if pipe else (op.flags | 1)
            kept = not pipe or self.opts["persist"] == 1
            self.tail_shape, self.slots, self.cur = shape, len(imgs), 0
            self.have_basis = kept
            self.have_orient = kept and bool(flags & 2)
            self.shape = shape if kept else None
            self.frames = [[(0, shape[0], (op, i, then))] for i in range(len(imgs))] if kept else []
            self.last_est = (not pipe, flags, shape, self.opts["layout"])

    @staticmethod
    def _cut(segs, lo, hi):
        for a, b, s in segs:
            if a < lo:
                yield (a, min(b, lo), s)
            if b > hi:
                yield (max(a, hi), b, s)

    def sources(self):
        """the row segments of the selected frame"""
        return self.frames[self.cur] if self.have_basis else []


# ---------------------------------------------------------------- the generator
def _pick_img(r, shape=None, u8=None):
    shape = r.choice(SHAPES) if shape is None else shape
    return (shape[0], shape[1], r.randrange(1000), (r.random() < 0.3) if u8 is None else u8)


def _gen_read_only(r, m, refuse=False, name=None):
    """one read-only call; refuse: one the model refuses where that is possible in its present state"""
    shape = m.shape or m.tail_shape or (8, 8)
    k4, ext = m.kind == 4, m.opts["g4_ext"] == 1
    n = name or r.choice([n for n in READ_ONLY if not (n == "steer_point" and k4)])
    full_ok = m.have_orient and not (k4 and not ext)
    if n in ("steer_scalar", "steer_map", "steer_bank"):
        full = r.random() < 0.5 and (full_ok or not m.have_basis)
        a = dict(full=full)
        if n != "steer_map":
            a["thetas" if n == "steer_bank" else "theta"] = ([round(r.uniform(-3, 3), 3) for _ in range(r.choice((1, 3)))] if n == "steer_bank"
                                                          else round(r.uniform(-3, 3), 3))
        if refuse and m.have_basis:
            if n != "steer_bank" and r.random() < 0.5:
                a["bad"] = "size"
            elif k4 and not ext:
                a["full"] = True      # G4 extras without CVS_OPT_G4_EXTENSIONS
        return Op(n, **a)
    if n == "steer_point":
        return Op(n, x=r.randrange(shape[1]), y=r.randrange(shape[0]), theta=round(r.uniform(-3, 3), 3))
    a = dict(shape=shape, seed=r.randrange(100))
    if refuse and m.have_orient:
        if r.random() < 0.5:
            a["shape"] = r.choice([s for s in SHAPES if s != shape])
        elif n == "nonmax":
            a["bad"] = "overlap"
    return Op(n, **a)


def _gen_establishing(r, m, name, refuse=False):
    k4, ext = m.kind == 4, m.opts["g4_ext"] == 1
    flags = r.choice((BASIS, FULL)) if (not k4 or ext) else BASIS
    if name in ("setup", "setup_pyr", "setup_steer"):
        a = dict(img=_pick_img(r, u8=False if name == "setup_pyr" else None), flags=flags)
        if name == "setup_steer":
            a["theta"] = round(r.uniform(-3, 3), 3)
        if refuse:
            if name == "setup_steer" and r.random() < 0.6:
                a["bad"] = r.choice(("size", "overlap"))
                if a["bad"] == "overlap":
                    a["img"] = a["img"][:3] + (False,)
            elif k4 and not ext:
                a["flags"] = FULL
        return Op(name, **a)
    if name == "setup_rows":
        # a band follows a whole-image call of the same size and flags; the caller (generate) has made sure of that
        shape, flags = m.last_est[2], m.last_est[1]
        lo = r.randrange(shape[0])
        return Op(name, img=_pick_img(r, shape), flags=flags, lo=lo, hi=r.randrange(lo + 1, shape[0] + 1))
    if name == "pipeline":
        subset = tuple(k for k in range(8) if r.random() < 0.6) or (5,)
        u8out = r.random() < 0.4
        if r.random() < 0.25:
            subset = (5, 6, 7)   # the three-maps launch
        a = dict(img=_pick_img(r), u8out=u8out, subset=subset, host=r.random() < 0.3)
        if refuse and (not k4 or ext):
            a["bad"] = r.choice(("size", "overlap"))
            a["img"], a["host"] = a["img"][:3] + (False,), False
        return Op(name, **a)
    shape, u8 = r.choice(SHAPES), r.random() < 0.3
    n = r.choice((1, 2, 2, 5, 5))
    imgs = tuple(_pick_img(r, shape, u8) for _ in range(n))
    if name == "pipeline_batch":
        subset = (5, 6, 7) if r.random() < 0.3 else (tuple(k for k in range(8) if r.random() < 0.5) or (0, 1))
        a = dict(imgs=imgs, scattered=r.random() < 0.6, u8out=r.random() < 0.3, subset=subset)
        if refuse and (not k4 or ext):
            a["bad"] = "size"
        return Op(name, **a)
    return Op(name, imgs=tuple(i[:3] + (u8 and name == "contours_batch",) for i in imgs))


def _gen_tail(r, m, name, refuse=False):
    shape = m.tail_shape or r.choice(SHAPES)
    if refuse and m.tail_shape is not None:
        shape = r.choice([s for s in SHAPES if s != m.tail_shape])   # a plane of another image's size
    a = dict(shape=shape, seed=r.randrange(100))
    if name in ("label", "contour_chains"):
        a["dense"] = r.random() < 0.5
    return Op(name, **a)


def generate(kind, seed, length):
    """the sequence of (kind, seed, length): deterministic, `length` steps, the last one a setup of an f32 image (the state the
    oracle check of run() reads)"""
    r = random.Random("%d/%d/%d" % (kind, seed, length))
    m = Model(kind)
    seq = []

    def emit(op):
        seq.append(op)
        if m.status(op) == OK:
            m.apply(op)

    if kind == 4 and r.random() < 0.75:
        emit(Op("set_option", opt="g4_ext", value=1))   # most G4 sequences start with the caller surface switched on
    names = [n for n in KINDS if n != "steer_point"] + (["steer_point"] * 2 if kind == 2 else []) + ["set_option"] * 3
    while len(seq) < length - 1:
        n = r.choice(names)
        refuse = r.random() < 0.22
        force = {}
        if m.have_basis and m.slots > 1 and m.cur == 0 and r.random() < 0.4:
            n, refuse = "select_frame", False    # histories that leave a frame other than 0 selected
        elif m.have_basis and m.opts["persist"] == 0 and m._caller_ok() and r.random() < 0.5:
            n, refuse = r.choice(("pipeline", "pipeline_batch")), False   # ... that run an outputs-only call over kept state
        elif seq and seq[-1].name == "set_u8_gain" and m._caller_ok() and r.random() < 0.6:
            n, refuse, force = "pipeline", False, dict(u8out=True)   # ... and that change the gain between two 8-bit calls
        elif n == "select_frame":
            refuse = r.random() < 0.4
        if n in READ_ONLY:
            op = _gen_read_only(r, m, refuse, n)
        elif n == "setup_rows":
            if not (m.last_est and m.last_est[0] and m.have_basis and m.slots == 1 and m.last_est[3] == m.opts["layout"]):
                if len(seq) >= length - 2:
                    continue
                emit(_gen_establishing(r, m, r.choice(("setup", "setup_steer", "setup_pyr"))))
                if not m.have_basis:
                    continue
            op = _gen_establishing(r, m, n)
        elif n in ESTABLISHING or n in TAIL_ESTABLISHING:
            if n == "contour_edgels_batch" and m.opts["persist"] == 0:
                # (the composite of the Python surface runs its pipeline_batch before its thinning finds no theta: not one refused call)
                if len(seq) >= length - 2:
                    continue
                emit(Op("set_option", opt="persist", value=1))
            op = _gen_establishing(r, m, n, refuse)
            op.a.update(force)
        elif n in TAIL:
            op = _gen_tail(r, m, n, refuse)
        elif n == "select_frame":
            i = r.randrange(m.slots > 1, m.slots) if m.have_basis and not refuse else r.choice((m.slots, m.slots, m.slots + 3, -1))
            op = Op(n, i=i)
        elif n == "read_state":
            op = Op(n, which=r.randrange(m.nb + 5))
        elif n == "basis_view":
            op = Op(n, p=r.randrange(m.nb))
        elif n == "set_option":
            opt = r.choice([o for o in OPTION_VALUES if o != "g4_ext"] + ["persist"] * 2 + ["g4_ext"] * (4 if kind == 4 else 0))
            value = r.choice(OPTION_VALUES[opt])
            if opt in ("g4_ext", "persist") and r.random() < 0.5:
                value = 1   # (most of the surface needs them on)
            op = Op(n, opt=opt, value=value)
        elif n == "set_u8_gain":
            op = Op(n, gain=r.choice(GAINS))
        elif n == "set_stream":
            op = Op(n, idx=r.randrange(2))
        elif n == "recreate":
            op = Op(n, shape=m.tail_shape or r.choice(SHAPES))
        else:
            op = Op(n)
        emit(op)
    k4_basis = kind == 4 and m.opts["g4_ext"] == 0
    emit(Op("setup", img=_pick_img(r, u8=False), flags=BASIS if (k4_basis or r.random() < 0.5) else FULL))
    return seq


# ---------------------------------------------------------------- the runner
class SequenceMismatch(AssertionError):
    def __init__(self, kind, seed, step, ops, detail, hip=False):
        self.kind, self.seed, self.step, self.ops, self.detail, self.hip = kind, seed, step, list(ops), detail, hip
        super().__init__("kind G%d seed %r step %d: %s\nreplay:\n  %s" % (kind, seed, step, detail, "\n  ".join(repr(o) for o in ops)))


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class _Run:
    def __init__(self, factory, kind, seed):
        self.factory, self.kind, self.seed = factory, kind, seed
        self.model = Model(kind)
        self.eng = factory(kind)
        self.done = []
        self.stats = dict(steps=0, refused=0, observations=0, planes=0, values=0, status_checks=0, twins=0, skipped=0)
        self.open = []

    def fail(self, detail, hip=False):
        raise SequenceMismatch(self.kind, self.seed, len(self.done) - 1, self.done, detail, hip)

    def issue(self, eng, op, who):
        st, res = eng.apply(op)
        if st == E_HIP:   # nothing further is issued on any engine
            self.open = []
            self.fail("HIP error in %s of the %s handle" % (op.name, who), hip=True)
        return st, res

    def set_options(self, eng, options, who):
        for k, v in options:
            op = Op("set_u8_gain", gain=v) if k == "gain" else Op("set_option", opt=k, value=v)
            if k == "g4_ext" and self.kind != 4:
                continue
            if self.issue(eng, op, who)[0] != OK:
                self.fail("%s refused %r" % (who, op))

    def twin(self, src, cache):
        """a fresh handle brought to the state of `src` by its recipe; (engine, what the establishing call returned)"""
        key = (src[0], src[1], src[2], self.model.options())
        if key not in cache:
            op, frame, then = src
            tw = self.factory(self.kind)
            self.open.append(tw)
            self.stats["twins"] += 1
            self.set_options(tw, then, "twin")
            st, res = self.issue(tw, op, "twin")
            if st != OK:
                self.fail("the twin refused its state-establishing call %r: %s" % (op, st))
            self.set_options(tw, self.model.options(), "twin")
            if frame and self.issue(tw, Op("select_frame", i=frame), "twin")[0] != OK:
                self.fail("the twin refused select_frame(%d)" % frame)
            cache[key] = (tw, res)
        return cache[key]

    def stitch(self, op, parts, shape):
        """expected result of `op`: rows [lo, hi) of every array from the twin that holds the state of those rows"""
        first = parts[0][2]
        if len(parts) == 1:
            return first
        out = []
        for k, a0 in enumerate(first):
            a = np.array(a0, copy=True)
            if op is not None and op.name == "chain_refine":
                ys = make_points(shape, op.seed)[:, 1]
                for lo, hi, res in parts:
                    sel = (ys >= lo) & (ys < hi)
                    a[sel] = res[k][sel]
            elif op is not None and op.name == "steer_point":
                for lo, hi, res in parts:
                    if lo <= op.y < hi:
                        a = np.array(res[k], copy=True)
            elif a.ndim >= 2 and tuple(a.shape[-2:]) == tuple(shape):
                for lo, hi, res in parts:
                    a[..., lo:hi, :] = res[k][..., lo:hi, :]
            out.append(a)
        return tuple(out)

    def compare(self, what, got, want):
        if len(got) != len(want):
            self.fail("%s: %d arrays, the twin has %d" % (what, len(got), len(want)))
        for k, (g, w) in enumerate(zip(got, want)):
            self.stats["values"] += int(np.asarray(w).size)
            if not _same(g, w):
                g, w = np.asarray(g), np.asarray(w)
                bad = int(np.count_nonzero(g.view(np.uint8) != w.view(np.uint8))) if g.shape == w.shape and g.dtype == w.dtype else -1
                self.fail("%s: array %d differs from the fresh twin (%s %s against %s %s, %d bytes)" % (what, k, g.shape, g.dtype, w.shape, w.dtype, bad))

    def read(self, op, cache):
        """issue a reading call on the long-lived handle and hold it against the model and the twin"""
        m = self.model
        want = m.status(op)
        got, res = self.issue(self.eng, op, "long-lived")
        self.stats["status_checks"] += 1
        if got != want:
            self.fail("%r returned %s, the contract says %s" % (op, got, want))
        if want != OK:
            return
        if op.name in ("hysteresis", "label", "link", "contour_chains", "contour_edgels"):
            # no handle state is read: the twin needs the image size only
            tw, _ = self.twin((Op("setup", img=(m.tail_shape[0], m.tail_shape[1], 0, False), flags=BASIS), 0, m.options()), cache)
            self.compare(repr(op), res, self.issue(tw, op, "twin")[1])
            return
        if op.name in ("select_frame", "set_option", "set_u8_gain", "set_stream"):
            return
        if op.name == "num_frames":
            return self.compare(repr(op), res, (np.int64(m.slots if m.have_basis else 0),))
        if op.name == "shape":
            return self.compare(repr(op), res, (np.array(m.shape or (0, 0), np.int64),))
        parts = []
        for lo, hi, src in m.sources():
            tw, _ = self.twin(src, cache)
            st, r = self.issue(tw, op, "twin")
            if st != OK:
                self.fail("the twin refused %r: %s" % (op, st))
            parts.append((lo, hi, r))
        self.compare(repr(op), res, self.stitch(op, parts, m.shape))

    def observe(self, cache, step):
        """every state plane of the selected frame, and one generated read-only call; without state: the model's status from every
        state-reading entry"""
        m = self.model
        self.stats["observations"] += 1
        got = self.eng.state()
        parts = []
        for lo, hi, src in m.sources():
            parts.append((lo, hi, self.twin(src, cache)[0].state()))
        for p in range(m.nb + 5):
            want = OK if (m.have_orient if p >= m.nb else m.have_basis) else E_STATE
            self.stats["status_checks"] += 1
            if got[p][0] == E_HIP:
                self.open = []
                self.fail("HIP error reading state plane %d" % p, hip=True)
            if got[p][0] != want:
                self.fail("state plane %d: status %s, the contract says %s" % (p, got[p][0], want))
            if want == OK:
                exp = self.stitch(None, [(lo, hi, (st[p][1],)) for lo, hi, st in parts], m.shape)
                self.stats["planes"] += 1
                self.compare("state plane %d of frame %d" % (p, m.cur), (got[p][1],), exp)
        r = random.Random("%d/%r/%d" % (self.kind, self.seed, step))
        if m.have_orient:
            self.read(_gen_read_only(r, m), cache)
        else:   # state missing, wholly or the orientation half: every state-reading entry answers as the model does
            shape = m.shape or m.tail_shape or (8, 8)
            ops = [Op("coefficients"), Op("basis_view", p=r.randrange(m.nb)), Op("steer_scalar", theta=0.3, full=False),
                   Op("steer_map", full=False), Op("steer_bank", thetas=[0.1, -0.7], full=False), Op("nonmax", shape=shape, seed=1),
                   Op("chain_refine", shape=shape, seed=1), Op("num_frames"), Op("shape")]
            if self.kind == 2:
                ops.append(Op("steer_point", x=0, y=0, theta=0.2))
            for op in ops:
                self.read(op, cache)

    def close(self, engines):
        for e in engines:
            if e in self.open:
                self.open.remove(e)
            e.close()

    def step(self, i, op):
        m = self.model
        self.done.append(op)
        self.stats["steps"] += 1
        cache = {}
        try:
            if op.name == "recreate":
                # a second live handle holds and releases blocks of the same sizes around the destroy / create of the long-lived
                # one: the state-block pool hands blocks over with work pending (one thread, two streams)
                other = self.factory(self.kind)
                self.open.append(other)
                self.issue(other, Op("set_stream", idx=1), "second")
                img = Op("setup", img=(op.shape[0], op.shape[1], 1, False), flags=BASIS)
                if self.issue(other, img, "second")[0] != OK:
                    self.fail("the second handle refused its setup")
                self.eng.close()
                self.eng = self.factory(self.kind)
                other.close()
                self.open.remove(other)
                m.apply(op)
                self.observe(cache, i)
                return
            if op.name in STATE_READS[1:] + READ_ONLY + TAIL[:5]:
                refused = m.status(op) != OK
                self.stats["refused"] += refused
                self.read(op, cache)
                if refused:
                    self.observe(cache, i)
                return
            want = m.status(op)
            got, res = self.issue(self.eng, op, "long-lived")
            self.stats["status_checks"] += 1
            if got != want:
                self.fail("%r returned %s, the contract says %s" % (op, got, want))
            if want == OK:
                m.apply(op)
                if res is not None and op.name != "setup_rows" and m.have_basis and m.frames[0][0][2][0] is op:
                    self.compare("outputs of %r" % (op,), res, self.twin(m.frames[0][0][2], cache)[1])
                elif res is not None and op.name in ("pipeline", "pipeline_batch"):   # no state kept: a twin for the outputs alone
                    self.compare("outputs of %r" % (op,), res, self.twin((op, 0, m.options()), cache)[1])
            else:
                self.stats["refused"] += 1
            self.observe(cache, i)
        finally:
            tw = [t for t, _ in cache.values()]
            cache.clear()
            if self.open is not None:
                self.close([t for t in tw if t in self.open])


def run(engine_factory, kind, sequence, seed=None, oracle=None, tol=1e-5):
    """Drive one long-lived engine through `sequence` (see the module docstring); raises SequenceMismatch at the first difference.
    oracle(kind, img) -> float64 [nb, rows, cols]: the last observation is also held to it, within tol, where basis state is valid.
    Returns the counters of the run; 'skipped' is the number of comparisons left out: always 0."""
    r = _Run(engine_factory, kind, seed)
    try:
        for i, op in enumerate(sequence):
            r.step(i, op)
        m = r.model
        if oracle is not None and m.have_basis:
            got = r.eng.state()
            planes = np.stack([got[p][1] for p in range(m.nb)]).astype(np.float64)
            for lo, hi, src in m.sources():
                o = src[0]
                img = (o.imgs if o.name in ("pipeline_batch",) + TAIL_ESTABLISHING else [o.img])[src[1]]
                if img[3]:
                    r.fail("the last state of a sequence comes from an f32 image (generator rule)")
                err = float(np.abs(planes[:, lo:hi] - oracle(kind, img)[:, lo:hi]).max())
                r.stats["oracle_err"] = max(r.stats.get("oracle_err", 0.0), err)
                if not err <= tol:
                    r.fail("basis planes rows %d..%d: %.3g from the oracle (bound %.3g)" % (lo, hi, err, tol))
    except SequenceMismatch as e:
        if not e.hip:
            r.close([r.eng] + list(r.open))
        raise
    r.close([r.eng] + list(r.open))
    return r.stats
