"""The float64 orientation model (orientation_model.py) and its input families, checked without a GPU: the oracle's float32 restatement
of the orientation stage is run on the families and held to the model at the very bounds tests/test_gpu_orientation.py asks of the
kernels, on every pixel, so the reference alone is shown to fit them; the families are shown to contain what they promise; and a
float32 emulation of the coefficient-table form shows that the bounds would catch a wrong kernel -- any single one of the 24 (G2) or 54
(G4) coefficients off by a factor 1 + 2^-10, swapped arctangent arguments, a lost wrap or * 0.5, the wrong arctangent.

Largest distances, oracle vs f64 (this module prints them).  `bound` is 1e-6 * max(1, (sum_G |b_i|)^2 + (sum_H |b_i|)^2) per pixel for
C1..C3 (orientation_model.bound), 1e-6 * max(1, hypot) for the strength; theta is held to 5e-6 rad on the stored C2, C3:
  family (taps)                  C1 / C2 / C3 (bound)     strength (bound)   theta, compatible / exact arctangent (rad)
  G2 impulses, step 9  (4, 0.67)   0.023 / 0.032 / 0.019    0.036              2.56e-7 / 1.76e-7
  G2 impulses, step 13 (6, 0.5)    0.020 / 0.034 / 0.032    0.059              2.60e-7 / 1.94e-7
  G2 mixed             (4, 0.67)   0.090 / 0.076 / 0.036    0.106              2.94e-7 / 2.58e-7
  G2 byte impulses     (4, 0.67)   0.055 / 0.072 / 0.038    0.109              2.96e-7 / 2.55e-7
  G4 impulses, step 13 (6, 0.5)    0.030 / 0.073 / 0.039    0.080              2.81e-7 / 2.15e-7
  G4 mixed             (6, 0.5)    0.103 / 0.141 / 0.070    0.108              2.90e-7 / 2.58e-7
Pixels with C3 == 0 != C2 / C2 == 0 != C3 / exact (0, 0): G2 step 9 20878 / 19641 / 34312, G4 step 13 14123 / 2184 / 42023;
max |C| 9.8e17 (G2), 1.0e18 (G4); smallest nonzero |(C2, C3)| 4.5e-29 (G2), 7.5e-37 (G4); no denormal C2 / C3, so the flush-to-zero
mode of a kernel cannot matter.
The net: the table emulation itself sits at 0.10 (G2) / 0.14 (G4) of the bound; with one coefficient scaled by 1 + 2^-10 the smallest
excess over all entries is 41.8 x the bound (G2) and 7.75 x (G4); the theta mutants miss by at least 1.43 rad (swapped arguments),
1.33 rad (lost wrap), 1.57 rad (lost * 0.5) and 8.3e-5 rad (the other arctangent, mixed family) on every family."""
import contextlib
import io
import os
import runpy
import sys
from fractions import Fraction

import numpy as np
import pytest

import angle_model as A
import orientation_model as O

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, kind, image, tap half-width, spacing)
FAMILIES = (("G2 impulses, step 9", 2, lambda: O.impulse_family(4), 4, 0.67),
            ("G2 impulses, step 13", 2, lambda: O.impulse_family(6), 6, 0.5),
            ("G2 mixed", 2, O.mixed_family, 4, 0.67),
            ("G2 byte impulses", 2, lambda: O.impulse_family_u8(4), 4, 0.67),
            ("G4 impulses, step 13", 4, lambda: O.impulse_family(6), 6, 0.5),
            ("G4 mixed", 4, O.mixed_family, 6, 0.5))


@pytest.fixture(scope="module")
def cases(ora):
    """name -> (kind, width, basis planes of the oracle, the model's C1..C3, bound): computed once, left unchanged"""
    out = {}
    for name, kind, make, w, s in FAMILIES:
        b = ora.basis(kind, make().astype(F32), w, s)
        out[name] = (kind, w, b, O.coefficients(b, kind), O.bound(b, kind))
    return out


def _orientation(ora, kind, b, exact=False):
    return (ora.g2_orientation if kind == 2 else ora.g4_orientation)(b, ora.ATAN_EXACT if exact else ora.ATAN_CV)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.mark.parametrize("exact", [False, True])
def test_oracle_fits_the_bounds(ora, cases, exact):
    for name, (kind, _, b, want, bd) in cases.items():
        c1, c2, c3, th, st = _orientation(ora, kind, b, exact)
        rc = [float((np.abs(got - w) / bd).max()) for got, w in zip((c1, c2, c3), want)]
        s = O.strength(c2, c3)
        rs = float((np.abs(st - s) / O.strength_bound(s)).max())
        dt = float(O.theta_error(th, O.theta(c2, c3, exact)).max())
        print("oracle vs f64, %s (exact=%s): C1..C3 error / bound %.3g %.3g %.3g, strength %.3g, theta %.3g rad" % ((name, exact) + tuple(rc) + (rs, dt)))
        assert max(rc) <= 1.0 and rs <= 1.0 and dt <= O.THETA_TOL, name


def test_families_hold_what_they_promise(ora, cases):
    for w in (4, 6):
        img = O.impulse_family(w)
        assert img.shape == (A.ROWS, A.COLS) and img.dtype == F32 and np.array_equal(img, O.impulse_family(w))
        ys, xs = np.nonzero(img)
        step = 2 * w + 1
        assert set(np.diff(np.unique(ys)).tolist()) == {step} and set(np.diff(np.unique(xs)).tolist()) == {step}   # no two supports overlap
        assert ys.min() == w and xs.min() == w and xs.max() + w < A.COLS and ys.max() + w < A.ROWS - O.ZERO_BAND
        amp = img[ys, xs]      # row-major order
        n = np.arange(amp.size)
        assert np.array_equal(amp, np.ldexp(np.where((n // 61) % 2 == 1, -1.0, 1.0), -30 + n % 61).astype(F32))
        assert amp.size > 2 * 61 and np.abs(amp).min() == 2.0 ** -30 and np.abs(amp).max() == 2.0 ** 30
        u8 = O.impulse_family_u8(w)
        assert u8.dtype == np.uint8 and np.array_equal(u8, O.impulse_family_u8(w))
        left = u8[:, :O.MIXED_BLOCKS[1]]
        assert np.array_equal(np.nonzero(left), np.nonzero(img[:, :O.MIXED_BLOCKS[1]])) and set(left[left != 0].tolist()) == set(O.U8_VALUES)
        assert len(set(u8[:, O.MIXED_BLOCKS[1]:].ravel().tolist())) == 256
    mixed = O.mixed_family()
    a, b_ = O.MIXED_BLOCKS
    assert mixed.shape == (A.ROWS, A.COLS) and mixed.dtype == F32 and np.array_equal(mixed, O.mixed_family())
    assert mixed[:, :a].max() > 200 and 0 <= mixed[:, a:b_].min() and mixed[:, a:b_].max() < 1
    assert np.abs(mixed[:, b_:]).max() > 2.0 ** 12 and np.abs(mixed[:, b_:]).min() < 2.0 ** -12 and (mixed[:, b_:] < 0).any()

    tiny = np.finfo(F32).tiny
    for name in ("G2 impulses, step 9", "G2 impulses, step 13", "G4 impulses, step 13"):
        kind, w, b, _, _ = cases[name]
        c1, c2, c3, th, st = _orientation(ora, kind, b)
        on_x, on_y, zz_n = O.axis_counts(c2, c3)
        hyp = O.strength(c2, c3)
        big, small = max(float(np.abs(c).max()) for c in (c1, c2, c3)), float(hyp[hyp > 0].min())
        print("%s: %d pixels with C3 == 0 != C2, %d with C2 == 0 != C3, %d exact (0, 0); max |C| %.3g, smallest nonzero |(C2, C3)| %.3g"
              % (name, on_x, on_y, zz_n, big, small))
        assert on_x >= 1000 and on_y >= 1000 and zz_n >= 10000
        assert big > 1e17 and small < 1e-20
        for c in (c2, c3):
            assert not ((c != 0) & (np.abs(c) < tiny)).any()          # no denormal: flush-to-zero cannot matter
        assert all(np.isfinite(p).all() for p in (c1, c2, c3, th, st))
        if kind == 2:
            z = np.signbit(c3[c3 == 0])
            assert z.any() and not z.all()                            # both signs of a zero C3
        band = O.zero_band(w)
        assert band.stop - band.start >= O.ZERO_BAND and all((c[band] == 0).all() for c in (c1, c2, c3))
        # (0, 0): strength is +0 and theta is 0; with the exact arctangent the sign of theta's zero is atan2's of the stored zeros
        zz = (c2 == 0) & (c3 == 0)
        assert not np.signbit(c2[zz]).any()
        assert (_bits(st)[zz] == 0).all() and (th[zz] == 0).all()
        th_x = _orientation(ora, kind, b, True)[3]
        assert (th_x[zz] == 0).all() and np.array_equal(np.signbit(th_x[zz]), np.signbit(c3[zz]))
        assert np.array_equal(np.signbit(np.arctan2(c3[zz], c2[zz])), np.signbit(c3[zz]))


# ---- the table form, emulated in float32: (i, j, which, k) adds k * (b_i * b_j) to C_which, every product and sum rounded ----
G2_TABLE = (  # the 24 constants of SteerableFiltersG2.cpp:93-95; planes g2a g2b g2c h2a h2b h2c h2d
    (1, 1, 1, 0.5), (0, 2, 1, 0.25), (0, 0, 1, 0.375), (2, 2, 1, 0.375), (3, 3, 1, 0.3125), (6, 6, 1, 0.3125), (4, 4, 1, 0.5625),
    (5, 5, 1, 0.5625), (3, 5, 1, 0.375), (4, 6, 1, 0.375),
    (0, 0, 2, 0.5), (2, 2, 2, -0.5), (3, 3, 2, 0.46875), (6, 6, 2, -0.46875), (4, 4, 2, 0.28125), (5, 5, 2, -0.28125), (3, 5, 2, 0.1875),
    (4, 6, 2, -0.1875),
    (0, 1, 3, -1.0), (1, 2, 3, -1.0), (5, 6, 3, -0.9375), (3, 4, 3, -0.9375), (4, 5, 3, -1.6875), (3, 6, 3, -0.1875))


def _tool_table(kind):
    """what tools/gen_g4_orient.py prints: lines `{i, j, which, num.f / den},`"""
    out, argv = io.StringIO(), sys.argv
    sys.argv = ["gen_g4_orient.py", "g%d" % kind]
    try:
        with contextlib.redirect_stdout(out):
            runpy.run_path(os.path.join(ROOT, "tools", "gen_g4_orient.py"), run_name="__main__")
    finally:
        sys.argv = argv
    table = []
    for line in out.getvalue().splitlines():
        i, j, which, k = line.strip().strip("{},").split(",")
        num, den = k.replace(".f", "").split("/")
        table.append((int(i), int(j), int(which), float(Fraction(int(num), int(den)))))
    return tuple(table)


def _terms(b, table):
    return [F32(k) * (b[i] * b[j]) for i, j, _, k in table]


def _sum(terms, table, which):
    v = np.zeros(terms[0].shape, F32)
    for t, (_, _, w, _) in zip(terms, table):
        if w == which:
            v = v + t
    assert v.dtype == F32
    return v


def test_the_net_is_fine_enough(cases):
    g4_table = _tool_table(4)
    assert len(G2_TABLE) == 24 and len(g4_table) == 54
    assert sorted(_tool_table(2)) == sorted(G2_TABLE)         # the tool's procedure reproduces the reference's constants
    up = 1.0 + 2.0 ** -10
    for kind, table in ((2, G2_TABLE), (4, g4_table)):
        fams = [(name, c) for name, c in cases.items() if c[0] == kind]
        terms = {name: _terms(c[2], table) for name, c in fams}
        as_written = 0.0
        for name, (_, _, b, want, bd) in fams:
            cs = [_sum(terms[name], table, w) for w in (1, 2, 3)]
            as_written = max(as_written, max(float((np.abs(c - w) / bd).max()) for c, w in zip(cs, want)))
            s = O.strength(cs[1], cs[2])
            st = np.sqrt(cs[1] * cs[1] + cs[2] * cs[2])
            assert st.dtype == F32 and float((np.abs(st - s) / O.strength_bound(s)).max()) <= 1.0
        assert as_written <= 1.0                              # the emulation passes as written
        weakest = np.inf
        for t, (i, j, which, k) in enumerate(table):
            assert float(F32(k * up)) == k * up               # the scaled coefficient is still a float32
            worst = 0.0
            for name, (_, _, b, want, bd) in fams:
                mutated = list(terms[name])
                mutated[t] = F32(k * up) * (b[i] * b[j])
                worst = max(worst, float((np.abs(_sum(mutated, table, which) - want[which - 1]) / bd).max()))
            assert worst > 1.0, (kind, t, table[t], worst)    # a coefficient off by 2^-10 is caught on at least one family
            weakest = min(weakest, worst)
        print("table emulation vs f64, G%d: as written %.3g bound; one coefficient * (1 + 2^-10): smallest excess %.3g x bound over %d entries"
              % (kind, as_written, weakest, len(table)))


def test_theta_mutants_exceed_the_tolerance(ora, cases):
    worst = {}
    for name, (kind, _, b, _, _) in cases.items():
        _, c2, c3, _, _ = _orientation(ora, kind, b)
        for exact in (False, True):
            atan = A.atan_0_2pi if exact else A.fast_atan_0_2pi
            other = A.fast_atan_0_2pi if exact else A.atan_0_2pi
            want = O.theta(c2, c3, exact)
            mutants = {"atan(C2, C3)": 0.5 * A.wrap(atan(c2, c3)), "no wrap": 0.5 * atan(c3, c2), "no * 0.5": A.wrap(atan(c3, c2)),
                       "the other arctangent": 0.5 * A.wrap(other(c3, c2))}
            for what, th in mutants.items():
                if what == "the other arctangent" and "mixed" not in name:   # the two differ by up to about 1e-4 rad: the mixed family shows it
                    continue
                d = float(O.theta_error(th.astype(F32), want).max())
                worst[what] = min(worst.get(what, np.inf), d)
                assert d > O.THETA_TOL, (name, exact, what, d)
    print("theta mutants, smallest miss over the families (rad): %s" % {k: "%.3g" % v for k, v in worst.items()})
