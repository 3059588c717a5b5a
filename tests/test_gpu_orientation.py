"""GPU test (-m gpu): the orientation stage -- C1..C3, strength = |(C2, C3)|, theta = wrap(atan(C3, C2)) / 2 (cvs_device_math.h:
g2_orientation, g4_orientation) -- of every launch that writes it, held to the table-free float64 model of tests/orientation_model.py
on every pixel: the epilogue of the G2 strip-kernel instances (full setup in every state layout, setup_steer, setup_pyr, the caller
pipeline with literal and with argument taps, the state-kept frame batch, a byte image, a generic width, both arctangents, streaming
stores), OP_G4_ORIENT and k_g4_pipeline.  Every launch is one call on a 131 x 1021 plane (frame batches: three or two of them), made
on a fresh handle and followed by a read-back of its own basis planes, C1..C3, theta and strength.

The comparisons are in the project's decoupled-stage form: C1..C3 against the model's projection of the launch's own basis planes,
strength and theta against the model on the launch's own C2, C3 -- so no pixel is masked out of anything.  Bounds (orientation_model):
1e-6 * max(1, (sum_G |b_i|)^2 + (sum_H |b_i|)^2) per pixel for C1..C3, 1e-6 * max(1, hypot) for the strength, 5e-6 rad for theta modulo
pi and within [-pi / 2, pi / 2].  The families (impulses 2^-30 .. 2^30 one tap support apart, a zero band; byte-range, unit-range and
2^-12 .. 2^12 noise) put thousands of pixels on either axis of the (C2, C3) plane with either sign of the zero, |C| from 1e-27 to
1e18, and exact (0, 0) pairs; each test asserts that the kernel's own planes contain them.

Largest distances (C1 / C2 / C3 and strength in bounds, theta in rad)   oracle vs f64 (test_orientation_model_cpu.py)   kernel vs f64 (MI355X)
  G2 impulses, step 9   compatible arctangent                            0.023 / 0.032 / 0.019, 0.036, 2.56e-7           0.023 / 0.032 / 0.019, 0.036, 2.56e-7 (every launch form)
  G2 mixed              compatible arctangent                            0.090 / 0.076 / 0.036, 0.106, 2.94e-7           0.089 / 0.070 / 0.043, 0.136, 2.97e-7 (every launch form)
  G2 both families      exact arctangent, theta                          1.76e-7 / 2.58e-7                               1.73e-7 / 2.57e-7
  G2 byte impulses                                                       0.055 / 0.072 / 0.038, 0.109, 2.96e-7           0.063 / 0.067 / 0.042, 0.132, 2.88e-7
  G2 impulses, step 13  taps (6, 0.5)                                    0.020 / 0.034 / 0.032, 0.059, 2.60e-7           0.020 / 0.034 / 0.032, 0.058, 2.60e-7
  G4 impulses, step 13  compatible / exact arctangent                    0.030 / 0.073 / 0.039, 0.080, 2.81e-7 / 2.15e-7 0.030 / 0.073 / 0.040, 0.091, 2.81e-7 / 1.79e-7
  G4 mixed              compatible / exact arctangent                    0.103 / 0.141 / 0.070, 0.108, 2.90e-7 / 2.58e-7 0.097 / 0.154 / 0.071, 0.130, 2.92e-7 / 2.57e-7"""
import numpy as np
import pytest
import torch

import angle_model as A
import cvsteer_amd as cv
import orientation_model as O
from cvsteer_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G2_TAPS, G4_TAPS = (4, 0.67), (6, 0.5)
GENERIC_TAPS = (6, 0.5)     # a G2 handle with these runs none of the width-4 instances


def _np(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _worst(r):
    """the largest of a plane of error / bound; a NaN (a kernel that lost a pixel) counts as a miss"""
    assert not np.isnan(r).any(), int(np.isnan(r).sum())
    return float(r.max())


@pytest.fixture(scope="module")
def images():
    """the families, on the device once: G2's (step 9) and G4's (step 13) impulses, the mixed plane, the byte impulses"""
    return {"impulses": _dev(O.impulse_family(4)), "impulses13": _dev(O.impulse_family(6)), "mixed": _dev(O.mixed_family()),
            "u8": _dev(O.impulse_family_u8(4))}


def _check(f, kind, what, exact=False, axes=None, band=None):
    """the state the last launch of handle f left, against the model of its own basis planes, on every pixel.  axes: the tap
    half-width of an impulse family -- the kernel's own C2, C3 must then hold the axis pixels; band: (rows, cols) slices where
    every plane must be an exact zero"""
    b = [_np(f.basis(p)) for p in range(7 if kind == 2 else 11)]
    c = [_np(x) for x in f.coefficients()]
    th, st = _np(f.getDominantOrientationAngle()), _np(f.getDominantOrientationStrength())
    assert all(p.shape == (A.ROWS, A.COLS) and p.dtype == np.float32 for p in b + c + [th, st])
    bd = O.bound(b, kind)
    rc = tuple(_worst(np.abs(got - want) / bd) for got, want in zip(c, O.coefficients(b, kind)))
    s = O.strength(c[1], c[2])
    rs = _worst(np.abs(st - s) / O.strength_bound(s))
    dt = _worst(O.theta_error(th, O.theta(c[1], c[2], exact)))
    print("kernel vs f64, %s: C1..C3 error / bound %.3g %.3g %.3g, strength %.3g, theta %.3g rad" % ((what,) + rc + (rs, dt)))
    assert max(rc) <= 1.0 and rs <= 1.0 and dt <= O.THETA_TOL, what
    if axes is not None:
        on_x, on_y, _ = O.axis_counts(c[1], c[2])
        assert on_x >= 1000 and on_y >= 1000, (what, on_x, on_y)
    if band is not None:
        assert band[0].stop - band[0].start >= O.ZERO_BAND
        for p in c + [th, st]:
            assert (p[band] == 0).all(), what
        assert (_bits(st)[band] == 0).all(), what     # strength is +0 at (0, 0)


def _bottom(width, cols=slice(None)):
    return (O.zero_band(width), cols)


def _family_checks(name, width=4):
    """the keyword arguments of _check for a G2 / G4 frame of the family `name`"""
    return dict(axes=width, band=_bottom(width)) if name.startswith("impulses") else {}


def _g2(opts=None, taps=G2_TAPS):
    f = cv.SteerableFiltersG2(None, *taps)
    for o, v in (opts or {}).items():
        f.set_option(o, v)
    return f


def _g4(exact=False):
    f = cv.SteerableFiltersG4(None, *G4_TAPS, extensions=True)
    f.set_atan_mode(exact)
    return f


# ----------------------------------------------------------------------------- G2: the strip-kernel epilogues
@pytest.mark.parametrize("family", ["impulses", "mixed"])
def test_g2_setup_in_every_state_layout(images, family):
    for opts, what in (({L.OPT_STATE_LAYOUT: 0}, "layout 0"), (None, "default layout"), ({L.OPT_STATE_LAYOUT: 2}, "layout 2"),
                       ({L.OPT_STATE_LAYOUT: 3}, "layout 3")):
        f = _g2(opts)
        f.setup(images[family], flags=cv.SETUP_FULL)
        _check(f, 2, "G2 setup(FULL), %s, %s" % (what, family), **_family_checks(family))


@pytest.mark.parametrize("family", ["impulses", "mixed"])
def test_g2_setup_steer_and_setup_pyr(images, family):
    f = _g2()
    f.setup_steer(images[family], 0.3, flags=cv.SETUP_FULL)
    _check(f, 2, "G2 setup_steer(FULL), %s" % family, **_family_checks(family))
    f = _g2()
    f.setup_pyr(images[family], flags=cv.SETUP_FULL)
    _check(f, 2, "G2 setup_pyr(FULL), %s" % family, **_family_checks(family))


@pytest.mark.parametrize("family", ["impulses", "mixed"])
def test_g2_pipeline_with_literal_and_argument_taps(images, family, monkeypatch):
    for lit in (1, 0):
        monkeypatch.setenv("CVS_OPTS", "lit=%d" % lit)
        f = _g2({L.OPT_AUTOTUNE: 0})
        f.pipeline(images[family])
        assert f.launch_info()["literal_taps"] == lit, f.launch_info()
        _check(f, 2, "G2 pipeline(), literal_taps=%d, %s" % (lit, family), **_family_checks(family))


def test_g2_pipeline_batch_of_three_frames(images):
    frames = torch.stack([images["impulses"], images["mixed"], torch.flip(images["impulses"], (0, 1))])
    f = _g2()
    f.pipeline_batch(frames)
    top = (slice(0, A.ROWS - O.zero_band(4).start), slice(None))     # the flipped frame's zero band
    for i, kw in enumerate((_family_checks("impulses"), {}, dict(axes=4, band=top))):
        f.select_frame(i)
        _check(f, 2, "G2 pipeline_batch, frame %d of 3" % i, **kw)


@pytest.mark.parametrize("family", ["impulses", "mixed"])
def test_g2_exact_arctangent(images, family):
    f = _g2()
    f.set_atan_mode(True)
    f.setup(images[family], flags=cv.SETUP_FULL)
    _check(f, 2, "G2 setup(FULL), exact arctangent, %s" % family, exact=True, **_family_checks(family))


def test_g2_byte_image(images):
    assert images["u8"].dtype == torch.uint8
    f = _g2()
    f.setup(images["u8"], flags=cv.SETUP_FULL)
    _check(f, 2, "G2 setup(FULL), byte impulses", axes=4, band=_bottom(4, slice(0, O.MIXED_BLOCKS[1] - 4)))
    f = _g2()
    f.pipeline(images["u8"])
    _check(f, 2, "G2 pipeline(), byte impulses", axes=4, band=_bottom(4, slice(0, O.MIXED_BLOCKS[1] - 4)))


def test_g2_generic_width(images):
    f = _g2(taps=GENERIC_TAPS)
    f.setup(images["impulses13"], flags=cv.SETUP_FULL)
    _check(f, 2, "G2 setup(FULL), taps (6, 0.5), impulses step 13", **_family_checks("impulses", 6))
    f = _g2(taps=GENERIC_TAPS)
    f.pipeline(images["impulses13"])
    _check(f, 2, "G2 pipeline(), taps (6, 0.5), impulses step 13", **_family_checks("impulses", 6))


@pytest.mark.parametrize("family", ["impulses", "mixed"])
def test_g2_streaming_stores_forced(images, family, monkeypatch):
    monkeypatch.setenv("CVS_OPTS", "nt_stores=1")
    f = _g2()
    f.setup(images[family], flags=cv.SETUP_FULL)
    assert f.launch_info()["nt_stores"] == 1
    _check(f, 2, "G2 setup(FULL), streaming stores, %s" % family, **_family_checks(family))
    f.pipeline(images[family])
    assert f.launch_info()["nt_stores"] == 1
    _check(f, 2, "G2 pipeline(), streaming stores, %s" % family, **_family_checks(family))


# ----------------------------------------------------------------------------- G4 with extensions: OP_G4_ORIENT and k_g4_pipeline
@pytest.mark.parametrize("exact", [False, True])
def test_g4_setup_and_pipeline(images, exact):
    for family in ("impulses13", "mixed"):
        f = _g4(exact)
        f.setup(images[family], flags=cv.SETUP_FULL)          # OP_G4_ORIENT
        _check(f, 4, "G4 setup(FULL), exact=%s, %s" % (exact, family), exact=exact, **_family_checks(family, 6))
        f = _g4(exact)
        f.pipeline(images[family])                           # k_g4_pipeline
        _check(f, 4, "G4 pipeline(), exact=%s, %s" % (exact, family), exact=exact, **_family_checks(family, 6))


def test_g4_pipeline_batch_of_two_frames(images):
    f = _g4()
    f.pipeline_batch(torch.stack([images["impulses13"], images["mixed"]]))
    for i, kw in enumerate((_family_checks("impulses13", 6), {})):
        f.select_frame(i)
        _check(f, 4, "G4 pipeline_batch, frame %d of 2" % i, **kw)
