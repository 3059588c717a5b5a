"""CPU test: the sequence harness of handle_sequences.py can fail.  A numpy surrogate engine implements the handle contract (every state
plane a cheap deterministic function of the image bytes, the plane index and the options; no filtering, because the runner compares an
engine with its own fresh twin only).  Eight one-line deviations can be injected into it; the committed seeds must catch each of them,
pass the faultless surrogate, and meet the coverage floor that any trimming of the GPU module has to keep."""
import collections

import numpy as np
import pytest

import handle_sequences as H
from handle_sequences import E_BADARG, E_SIZE, E_STATE, E_UNSUPPORTED, OK

FAULTS = ("orient_kept", "cur_frame_kept", "select_accepts_n", "persist_off_keeps_basis", "refused_clears", "scatter_misfiled",
          "band_disturbs", "gain_of_previous_call")


class Surrogate:
    """the handle contract in numpy, written on its own (it shares the input generators with the model, not its logic)"""

    def __init__(self, kind, fault=None):
        self.kind, self.nb, self.fault = kind, H.NB[kind], fault
        self.o = dict(H.OPTION_DEFAULTS)
        self.gain = self.gain_prev = 0.0
        self.basis = self.orient = False
        self.size = None        # image size of the handle (the contour tail's)
        self.frames = []        # state block: grown, never cleared
        self.n = 1
        self.cur = 0

    def close(self):
        self.frames = None

    # -- state
    def planes(self, img, full):
        base = H.make_image(img).astype(np.float32)
        ps = [base * np.float32(p + 1) + np.float32(p) for p in range(self.nb)]
        for q in range(5):
            ps.append(base * np.float32(q + 2) - np.float32(0.25 * self.o["atan"]) if full else np.full(base.shape, np.nan, np.float32))
        return np.stack(ps)

    def frame(self):
        return self.frames[min(self.cur, len(self.frames) - 1)]

    def state(self):
        out = []
        for p in range(self.nb + 5):
            ok = self.orient if p >= self.nb else self.basis
            out.append((OK, self.frame()[p].copy()) if ok else (E_STATE, None))
        return out

    def establish(self, imgs, full, keep=True, misfile=False):
        shape = tuple(imgs[0][:2])
        new = [self.planes(i, full) for i in imgs]
        self.size = shape
        if not keep:
            if self.fault != "persist_off_keeps_basis":
                self.basis = self.orient = False
            self.n = len(imgs)
            return new
        if full or self.fault != "orient_kept":
            self.orient = full
        # (a frame table left over from an earlier call: a fresh handle files its frames correctly)
        stored = new[1:] + new[:1] if (misfile and self.fault == "scatter_misfiled" and self.frames) else new
        self.frames = stored + self.frames[len(new):]
        if not (self.fault == "cur_frame_kept" and len(new) < self.n):
            self.cur = 0
        self.n = len(imgs)
        self.basis = True
        return new

    # -- outputs
    def to_u8(self, a):
        g = self.gain_prev if self.fault == "gain_of_previous_call" else self.gain
        if g > 0:
            return np.clip(np.rint(a * np.float32(g)), 0, 255).astype(np.uint8)
        lo, hi = float(a.min()), float(a.max())
        return np.rint((a - lo) * (255.0 / (hi - lo) if hi > lo else 0.0)).astype(np.uint8)

    def maps(self, planes, subset, u8):
        outs = [planes[k % (self.nb + 5)] * np.float32(1 + (self.o["find_on"] if k >= 5 else 0)) for k in subset]
        return [self.to_u8(a) if u8 else a for a in outs]

    def steer(self, theta, full):
        s = self.frame()
        c, sn = np.float32(np.cos(theta)), np.float32(np.sin(theta))
        out = [s[0] * c + s[1] * sn, s[self.nb - 1] * c]
        if full:
            out += [s[self.nb] * c, s[self.nb + 1] + sn, s[self.nb + 2] * np.float32(1 + self.o["atan"])]
        return out

    def caller(self):
        return self.kind == 2 or self.o["g4_ext"] == 1

    def apply(self, op):
        st, res = self.call(op)
        if st != OK and self.fault == "refused_clears":
            self.basis = self.orient = False
        return st, (tuple(np.asarray(r) for r in res) if res is not None else None)

    def call(self, op):
        n, bad, k4 = op.name, op.get("bad"), self.kind == 4
        refusal = {None: None, "size": E_SIZE, "overlap": E_BADARG}[bad]
        if n == "set_option":
            self.o[op.opt] = op.value
            return OK, ()
        if n == "set_u8_gain":
            self.gain = op.gain
            return OK, ()
        if n == "set_stream":
            return OK, ()
        if n in ("setup", "setup_steer", "setup_pyr", "setup_rows"):
            full = bool(op.flags & 2)
            if full and k4 and (n == "setup_rows" or not self.o["g4_ext"]):
                return E_UNSUPPORTED, None
            if refusal:
                return refusal, None
            if n == "setup_rows" and not H.generic_path(self.kind, tuple(op.img[:2])):
                new, f = self.planes(op.img, full), self.frames[0]
                top = self.nb + 5 if full else self.nb
                f[:top, op.lo:op.hi] = new[:top, op.lo:op.hi]
                if self.fault == "band_disturbs" and op.hi < f.shape[1]:
                    f[:top, op.hi] = new[:top, op.hi]
                self.cur, self.basis, self.orient = 0, True, full
                return OK, ()
            self.establish([op.img], full)
            if n == "setup_steer":
                return OK, self.steer(op.theta, False)
            if n == "setup_pyr":
                return OK, [H.make_image(op.img)[::2, ::2].astype(np.float32)]
            return OK, ()
        if n in ("pipeline", "pipeline_batch", "contours_batch", "contour_edgels_batch"):
            if not self.caller():
                return E_UNSUPPORTED, None
            if n.startswith("contour") and not self.o["persist"]:
                return E_STATE, None
            if refusal:
                return refusal, None
            imgs = [op.img] if n == "pipeline" else list(op.imgs)
            new = self.establish(imgs, True, keep=self.o["persist"] == 1, misfile=len(imgs) > 1 and op.get("scattered", False))
            subset, u8 = (op.subset, op.u8out) if n.startswith("pipeline") else ((5, 6, 7), True)
            res = [np.stack(self.maps(p, subset, u8)) for p in new]
            self.gain_prev = self.gain
            return OK, (res if n == "pipeline" else [np.stack(res)])
        if n == "select_frame":
            top = self.n + (1 if self.fault == "select_accepts_n" else 0)
            if not 0 <= op.i < top:
                return E_BADARG, None
            self.cur = op.i
            return OK, ()
        if n == "num_frames":
            return OK, [np.int64(self.n if self.basis else 0)]
        if n == "shape":
            return OK, [np.array(self.frame().shape[1:] if self.basis else (0, 0), np.int64)]
        if n == "read_state":
            st = self.state()[op.which]
            return st[0], ([st[1]] if st[0] == OK else None)
        if n == "coefficients":
            return (OK, list(self.frame()[self.nb:self.nb + 3])) if self.orient else (E_STATE, None)
        if n == "basis_view":
            return (OK, [np.array(self.frame().shape[1:], np.int64), self.frame()[op.p]]) if self.basis else (E_STATE, None)
        if n in ("steer_scalar", "steer_map", "steer_bank"):
            if not self.basis:
                return E_STATE, None
            if refusal:
                return refusal, None
            if op.full and k4 and not self.o["g4_ext"]:
                return E_UNSUPPORTED, None
            if (op.full or n == "steer_map") and not self.orient:
                return E_STATE, None
            if n == "steer_map":
                return OK, [a + self.frame()[self.nb + 3] for a in self.steer(0.5, op.full)]
            if n == "steer_bank":
                return OK, [np.stack(k) for k in zip(*[self.steer(t, op.full) for t in op.thetas])]
            return OK, self.steer(op.theta, op.full)
        if n == "steer_point":
            if k4:
                return E_UNSUPPORTED, None
            if not self.basis:
                return E_STATE, None
            v = [a[op.y, op.x] for a in self.steer(op.theta, self.orient)]
            return OK, [np.array(v + [np.nan] * (5 - len(v)), np.float32)]
        if n in ("nonmax", "chain_refine"):
            if not (self.basis and self.orient):
                return E_STATE, None
            if tuple(op.shape) != self.frame().shape[1:]:
                return E_SIZE, None
            if refusal:
                return refusal, None
            m, th = H.make_map(tuple(op.shape), op.seed), self.frame()[self.nb + 3]
            if n == "nonmax":
                return OK, [np.where(th > np.float32(1.0), m, np.float32(0))]
            pts = H.make_points(tuple(op.shape), op.seed)
            return OK, [pts.astype(np.float32) + th[pts[:, 1], pts[:, 0]][:, None], m[pts[:, 1], pts[:, 0]] * self.frame()[self.nb + 4][pts[:, 1], pts[:, 0]]]
        if n in ("hysteresis", "label", "link", "contour_chains", "contour_edgels"):
            if self.size is None:
                return E_STATE, None
            if tuple(op.shape) != self.size:
                return E_SIZE, None
            if n in ("label", "contour_chains"):
                return OK, [np.cumsum(H.make_mask(self.size, op.seed, op.dense) > 0).astype(np.int32)]
            return OK, [(H.make_map(self.size, op.seed) > np.float32(H.HIGH)).astype(np.uint8) * np.uint8(255)]
        raise ValueError(n)


def _sequences(kind):
    return [(s, H.generate(kind, s, H.LENGTH)) for s in H.COMMITTED[kind]]


def _factory(fault=None):
    return lambda kind: Surrogate(kind, fault)


def _caught(kind, fault):
    """the committed seeds of `kind` whose sequence stops on the fault, with the step"""
    hits = []
    for seed, seq in _sequences(kind):
        try:
            H.run(_factory(fault), kind, seq, seed)
        except H.SequenceMismatch as e:
            assert e.kind == kind and e.seed == seed and e.ops == seq[:e.step + 1]   # enough to replay the case by hand
            hits.append((seed, e.step))
    return hits


def test_generator_is_deterministic():
    for kind in (2, 4):
        a, b = H.generate(kind, 3, H.LENGTH), H.generate(kind, 3, H.LENGTH)
        assert len(a) == H.LENGTH and [repr(o) for o in a] == [repr(o) for o in b]
        assert [repr(o) for o in a] != [repr(o) for o in H.generate(kind, 4, H.LENGTH)]
        assert eval(repr(a[0]), {"Op": H.Op}) == a[0]   # a reported operation list is Python


@pytest.mark.parametrize("kind", (2, 4))
def test_faultless_surrogate_passes_every_committed_sequence(kind):
    for seed, seq in _sequences(kind):
        stats = H.run(_factory(), kind, seq, seed, oracle=lambda k, img: Surrogate(k).planes(img, False)[:H.NB[k]].astype(np.float64))
        assert stats["steps"] == H.LENGTH and stats["skipped"] == 0 and stats["observations"] > 0 and stats["planes"] > 0
        assert stats["oracle_err"] == 0.0


@pytest.mark.parametrize("fault", FAULTS)
def test_every_injected_fault_is_caught(fault):
    g2, g4 = _caught(2, fault), _caught(4, fault)
    print(fault, "G2", g2, "G4", g4)
    assert len(g2) >= 3, g2
    assert len(g4) >= 1, g4   # (every fault applies to G4 handles as well: with CVS_OPT_G4_EXTENSIONS they have the whole caller surface)


def test_oracle_check_of_the_last_observation_can_fail():
    seed, seq = _sequences(2)[0]
    with pytest.raises(H.SequenceMismatch, match="from the oracle"):
        H.run(_factory(), 2, seq, seed, oracle=lambda k, img: Surrogate(k).planes(img, False)[:7].astype(np.float64) + 1e-4)


def test_committed_sequences_cover_the_alphabet():
    count, pairs, shapes, refused, steps = collections.Counter(), set(), collections.Counter(), 0, 0
    for kind in (2, 4):
        for seed, seq in _sequences(kind):
            m, prev = H.Model(kind), None
            for op in seq:
                count[op.name] += 1
                steps += 1
                st = m.status(op)
                refused += st != OK
                if st == OK:
                    if op.name in H.ESTABLISHING:
                        pairs.add((prev, op.name))
                        prev = op.name
                    if op.name in H.ESTABLISHING + H.TAIL_ESTABLISHING:
                        shapes[tuple((op.imgs[0] if "imgs" in op.a else op.img)[:2])] += 1
                    m.apply(op)
    print(sorted(count.items(), key=lambda kv: kv[1]), refused / steps, sorted(shapes.items()))
    assert set(count) == set(H.KINDS)
    assert min(count.values()) >= 20, min(count.items(), key=lambda kv: kv[1])
    # a band is defined only behind a whole-image setup of the same flags (handle_sequences.py, cvs_setup_rows in the header): the
    # caller pipeline has no flags, so no sequence may put cvs_setup_rows straight behind cvs_pipeline / cvs_pipeline_batch
    want = {(a, b) for a in H.ESTABLISHING for b in H.ESTABLISHING} - {("pipeline", "setup_rows"), ("pipeline_batch", "setup_rows")}
    assert want <= pairs, sorted(want - pairs)
    assert set(shapes) == set(H.SHAPES) and min(shapes.values()) >= 5, shapes
    assert refused >= 0.15 * steps, (refused, steps)
    # every option value and every refusal kind occurs
    opts = {(op.opt, op.value) for kind in (2, 4) for _, seq in _sequences(kind) for op in seq if op.name == "set_option"}
    assert opts >= {(o, v) for o, vs in H.OPTION_VALUES.items() for v in vs}
    bads = {(op.name, op.get("bad")) for kind in (2, 4) for _, seq in _sequences(kind) for op in seq if op.get("bad")}
    assert {b for _, b in bads} == {"size", "overlap"}
