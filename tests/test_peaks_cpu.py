"""Orientation peaks (cvs_orientation_peaks) at every layer that exists without a GPU: the header, the binding, the facade's exports, the
Python surface, the generated code of the kernel instances -- and the rules themselves: the float32 model of tests/peaks_model.py on
hand-made energies, on the oracle's basis planes of known structures, and against the float64 model."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import peaks_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "cvsteer_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
F32 = np.float32
PI_F = F32(np.pi)


# ---- the layers ----
def test_header_declares_the_call_and_its_struct():
    text = open(os.path.join(ROOT, "include", "cvsteer_hip.h")).read()
    assert re.search(r"#define CVS_PEAKS_MAX 4\b", text)
    assert re.search(r"typedef struct cvs_peaks_cfg \{\s*unsigned struct_size;[^}]*int n_angles;[^}]*int max_peaks;[^}]*float min_energy;"
                     r"[^}]*float min_ratio;[^}]*float min_contrast;[^}]*\} cvs_peaks_cfg;", text)
    assert re.search(r"int cvs_orientation_peaks\(cvs_handle h, const cvs_peaks_cfg\* cfg,\s*const cvs_plane\* angles,[^;]*"
                     r"const cvs_plane\* energies,[^;]*const cvs_plane\* count\);", text)
    assert re.search(r"#define CVS_ABI_VERSION 2\b", text)   # additive


def test_binding_has_the_call_and_the_struct():
    from cvsteer_amd import _lib as L
    res, args = L.SIGNATURES["cvs_orientation_peaks"]
    assert res is C.c_int
    assert args == [C.c_void_p, C.POINTER(L.PeaksCfg), C.POINTER(L.Plane), C.POINTER(L.Plane), C.POINTER(L.Plane)]
    assert [n for n, _ in L.PeaksCfg._fields_] == ["struct_size", "n_angles", "max_peaks", "min_energy", "min_ratio", "min_contrast"]
    assert C.sizeof(L.PeaksCfg) == 24 and L.PEAKS_MAX == 4
    assert L.lib().cvs_orientation_peaks.argtypes == args   # exported by the built library


def test_python_classes_have_orientation_peaks():
    import cvsteer_amd
    for cls in (cvsteer_amd.SteerableFiltersG2, cvsteer_amd.SteerableFiltersG4):
        assert callable(getattr(cls, "orientation_peaks", None)), cls


def test_facade_exports_orientation_peaks():
    so = os.path.join(ROOT, "cvsteer_amd", "libcvsteer.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cvsteer_amd", "facade"), "-s"])
    syms = subprocess.check_output(["nm", "-DC", "--defined-only", so], text=True)
    vm = "std::vector<fa::Mat1f, std::allocator<fa::Mat1f> >&"
    for cls in ("SteerableFiltersG2", "SteerableFiltersG4"):
        needle = "fa::%s::orientationPeaks(%s, %s, int, int, float, float, float)" % (cls, vm, vm)
        assert needle in syms, needle


def test_a_null_handle_is_refused_without_a_device():
    from cvsteer_amd import _lib as L
    cfg = L.PeaksCfg(C.sizeof(L.PeaksCfg), 16, 2, 0.0, 0.25, 1e-3)
    planes = (L.Plane * 2)()
    assert L.lib().cvs_orientation_peaks(None, C.byref(cfg), planes, planes, None) == L.E_BADARG


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_peaks_instances_use_no_scratch(tmp_path):
    """all eight k_orientation_peaks instances (G2 / G4 x float4 / dword x a list of two / four) keep the samples, the range and the
    list in registers: no private segment"""
    path = os.path.join(str(tmp_path), "cvs_kernels_peaks.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    "-I" + SRC, "-S", "--cuda-device-only", os.path.join(SRC, "cvs_kernels_peaks.hip"), "-o", path], check=True, stderr=subprocess.DEVNULL)
    text = open(path).read()
    scratch = {}
    for blk in text.split("  - .agpr_count:")[1:]:
        nm = re.search(r"\.name:\s+(\S+)", blk)
        ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        if nm and ps:
            scratch[nm.group(1)] = int(ps.group(1))
    inst = {n: s for n, s in scratch.items() if "k_orientation_peaks" in n}
    assert len(inst) == 8, sorted(inst)
    assert len({n for n in inst if "ILi7E" in n}) == 4 and len({n for n in inst if "ILi11E" in n}) == 4
    assert all(s == 0 for s in inst.values()), inst


# ---- the rules on hand-made energies: e[K] at one pixel ----
def _one(e, M=4, me=0.0, mr=0.0, mc=0.0):
    a, en, c = pm.peaks_f32(np.asarray(e, F32).reshape(-1, 1, 1), M, me, mr, mc)
    return a[:, 0, 0], en[:, 0, 0], int(c[0, 0])


def _ks(a, K):
    """sample index nearest to each angle"""
    return [int(round(float(x) / (np.pi / K))) % K if x >= 0 else -1 for x in a]


def test_a_two_sample_plateau_keeps_one_sample():
    a, en, c = _one([1, 2, 5, 5, 2, 1, 1, 1])
    assert c == 1
    # k = 2 survives (e_2 > e_1 && e_2 >= e_3); k = 3 does not (e_3 > e_2 fails); the parabola through (2, 5, 5) moves it half a step
    assert a[0] == F32(F32(2.5) * pm.step_f32(8)) and en[0] == F32(5.375)


def test_ties_are_ordered_by_k_and_wrap_around_peaks_count():
    K = 8
    a, en, c = _one([7, 1, 1, 7, 1, 1, 1, 3], M=4)   # k = 0 and k = 3 tie; k = 7 rises from e_6 but lies below e_0: no candidate
    assert c == 2 and _ks(a, K)[:2] == [0, 3]
    a, en, c = _one([1, 1, 6, 1, 1, 6, 1, 6])       # k = 2, 5, 7 tie: ascending k; k = 7 peaks across the wrap (e_0 = 1)
    assert c == 3 and _ks(a, K)[:3] == [2, 5, 7]
    a, en, c = _one([6, 1, 2, 1, 1, 1, 1, 5])       # k = 0 peaks against e_7 = 5 and e_1 = 1
    assert c == 2 and _ks(a, K)[0] in (0, 7) and en[0] > 6
    assert _ks(a, K)[1] == 2


def test_angles_land_in_zero_pi():
    K = 8
    # a peak at k = 0 pulled below zero by its left neighbour wraps to just under pi; one at k = K - 1 pulled up stays below pi
    a, _, c = _one([6, 1, 1, 1, 1, 1, 1, 5])
    assert c == 1 and 0 <= a[0] < PI_F and a[0] > F32(3.0)
    a, _, c = _one([5.5, 1, 1, 1, 1, 1, 1, 6])
    assert c == 1 and 0 <= a[0] < PI_F and a[0] > F32(2.7)
    rng = np.random.default_rng(0)
    e = rng.random((16, 40, 50)).astype(F32)
    a, en, c = pm.peaks_f32(e, 4)
    used = a >= 0
    assert (a[used] < PI_F).all() and used.sum() == int(c.sum())


def test_unused_slots_and_saturation():
    a, en, c = _one([1, 5, 1, 4, 1, 3, 1, 2], M=4)
    assert c == 4 and _ks(a, 8) == [1, 3, 5, 7]
    a, en, c = _one([1, 5, 1, 4, 1, 3, 1, 2], M=2)   # count saturates at M, the strongest stay
    assert c == 2 and _ks(a, 8) == [1, 3]
    a, en, c = _one([1, 5, 1, 1, 1, 1, 1, 1], M=4)
    assert c == 1 and list(a[1:]) == [F32(-1)] * 3 and list(en[1:]) == [F32(0)] * 3


def test_flat_and_non_finite_pixels_have_no_peaks():
    assert _one([3] * 8)[2] == 0
    assert _one([0] * 8)[2] == 0
    for bad in (np.nan, np.inf):
        a, en, c = _one([1, 5, 1, bad, 1, 3, 1, 2])
        assert c == 0 and (a == F32(-1)).all() and (en == 0).all()


def test_each_threshold_at_equality():
    e = [1, 8, 1, 4, 1, 1, 1, 1]                     # peaks 8 (k = 1) and 4 (k = 3); emax 8, emin 1
    up, down = np.nextafter(F32(4), F32(9)), np.nextafter(F32(4), F32(0))
    # e_k > min_energy: strict
    assert _one(e, me=float(down))[2] == 2 and _one(e, me=4.0)[2] == 1 and _one(e, me=float(up))[2] == 1
    # e_k >= min_ratio * emax: 4 >= 0.5 * 8 holds at equality
    assert _one(e, mr=0.5)[2] == 2 and _one(e, mr=float(np.nextafter(F32(0.5), F32(1))))[2] == 1
    assert _one(e, mr=float(np.nextafter(F32(0.5), F32(0))))[2] == 2
    # emax - emin > min_contrast * emax: strict; 8 - 1 = 7 = 0.875 * 8
    assert _one(e, mc=0.875)[2] == 0 and _one(e, mc=float(np.nextafter(F32(0.875), F32(0))))[2] == 2
    assert _one(e, mc=float(np.nextafter(F32(0.875), F32(1))))[2] == 0


# ---- known answers on the oracle's basis planes ----
WIDTH = {2: (4, 0.67), 4: (6, 0.5)}


def _oracle_energies(ora, kind, img, K):
    b = ora.basis(kind, img, *WIDTH[kind])
    out = []
    for th in pm.sample_angles(K):
        g, h = (ora.g2_steer_scalar(b, float(th))[:2] if kind == 2 else ora.g4_steer_scalar(b, float(th)))
        out.append((g * g + h * h).astype(F32))
    return np.stack(out), b


def _deg_err(angle, want_deg):
    d = abs(float(np.rad2deg(angle)) - want_deg) % 180.0
    return min(d, 180.0 - d)


RIDGE_BOUND, CROSS_BOUND = pm.RIDGE_BOUND, pm.CROSS_BOUND   # twice what the model measures here: the figures stand in peaks_model.py


@pytest.mark.parametrize("kind", [2, 4])
@pytest.mark.parametrize("K", [8, 16, 32])
def test_one_ridge_peaks_across_its_direction(ora, kind, K):
    worst = 0.0
    for phi in (0, 20, 45, 77, 90, 130):
        e, _ = _oracle_energies(ora, kind, pm.ridge_image([phi]), K)
        a, en, c = pm.peaks_f32(e, 2, 0.0, 0.25, 1e-3)
        assert c[24, 24] == 1, (phi, c[24, 24])
        worst = max(worst, _deg_err(a[0, 24, 24], phi + 90.0))
    print("kind %d K %d: worst angle error %.4f deg (bound %.4f)" % (kind, K, worst, RIDGE_BOUND[(kind, K)]))
    assert worst <= RIDGE_BOUND[(kind, K)]


def test_g4_resolves_the_perpendicular_crossing_and_g2_needs_the_contrast_rule(ora):
    img = pm.ridge_image([20, 110])
    e4, _ = _oracle_energies(ora, 4, img, 16)
    a, en, c = pm.peaks_f32(e4, 4, 0.0, 0.5, 1e-3)
    assert c[24, 24] == 2
    errs = sorted(min(_deg_err(x, 110.0), _deg_err(x, 20.0)) for x in a[:2, 24, 24])
    arms = sorted(round(float(np.rad2deg(x)) / 90.0) for x in a[:2, 24, 24])
    print("G4 crossing: arm errors %s deg (bound %.4f)" % (errs, CROSS_BOUND))
    assert arms == [0, 1] and errs[1] <= CROSS_BOUND
    e2, _ = _oracle_energies(ora, 2, img, 16)
    assert pm.peaks_f32(e2, 4, 0.0, 0.5, 1e-3)[2][24, 24] == 0       # flat to rounding: no orientation to report
    assert pm.peaks_f32(e2, 4, 0.0, 0.5, 0.0)[2][24, 24] > 0         # ... and rounding noise reported as peaks without the rule


# ---- float32 against float64 ----
# (the tolerances: peaks_model.F64_ANGLE_TOL / F64_ENERGY_TOL, four times the worst difference this test measures over its twelve cases)
F64_ANGLE_TOL, F64_ENERGY_TOL = pm.F64_ANGLE_TOL, pm.F64_ENERGY_TOL


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("kind", [2, 4])
def test_float32_model_against_float64(ora, kind, seed):
    img = pm.smoothed_noise(64, 96, seed)
    for K in (8, 16, 32):
        e, b = _oracle_energies(ora, kind, img, K)
        a32, e32, c32 = pm.peaks_f32(e, 4)
        a64, e64, c64, thin = pm.peaks_f64(b, kind, K, 4)
        frac = float(thin.mean())
        assert frac <= 0.01, frac                                   # a condition of the comparison, not a result
        assert np.array_equal(c32[~thin], c64[~thin])
        da, de = pm.match_sets(a32, e32, np.where(thin, 0, c32), a64, e64, np.where(thin, 0, c64))
        print("kind %d seed %d K %d: thin %.4f, angle %.3g rad, energy %.3g, most peaks %d" % (kind, seed, K, frac, da, de, int(c32.max())))
        assert da <= F64_ANGLE_TOL and de <= F64_ENERGY_TOL
