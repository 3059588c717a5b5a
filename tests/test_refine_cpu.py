"""Contour edgels (cvs_chain_refine, cvs_chain_measures) at every layer that exists without a GPU: the public header, the exports of both
libraries, the Python surface, the generated code of the new kernels (no scratch), and the models of refine_model.py that the GPU tests hold
the kernels against -- the contract's own consequences (|t| <= 0.5, t = 0 and strength == m where the keep test fails), the geometry of
straight ridges, and the measures against a second, vectorised computation."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import chains_model as CM
import contour_model as NM
import refine_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "cvsteer_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
F32 = np.float32


def test_header_declares_the_calls_and_the_record(tmp_path):
    text = open(os.path.join(ROOT, "include", "cvsteer_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int cvs_chain_refine\(cvs_handle h, const cvs_plane\* map, const cvs_plane\* theta,\s*const int32_t\* points, int n_points,\s*"
                     r"float\* xy,\s*float\* strength,\s*int mem\);", plain)
    assert re.search(r"int cvs_chain_measures\(cvs_handle h, const int32_t\* points, int n_points,\s*const cvs_chain\* chains, int n_chains,\s*"
                     r"const float\* xy,\s*const float\* strength,\s*cvs_chain_measure\* table, int mem\);", plain)
    assert re.search(r"#define CVS_ABI_VERSION 2\b", text)
    assert "UN-THINNED" in text                                               # the header says which map the call wants
    src = os.path.join(str(tmp_path), "use.cpp")
    with open(src, "w") as f:
        f.write('#include <stddef.h>\n#include "cvsteer_hip.h"\n'
                'static_assert(sizeof(cvs_chain_measure) == 40, "40 bytes");\n'
                'static_assert(offsetof(cvs_chain_measure, peak_index) == 12 && offsetof(cvs_chain_measure, weakest) == 20, "ints, floats");\n'
                'static_assert(offsetof(cvs_chain_measure, sum) == 24 && offsetof(cvs_chain_measure, length) == 32, "doubles");\n'
                'int (*refine)(cvs_handle, const cvs_plane*, const cvs_plane*, const int32_t*, int, float*, float*, int) = cvs_chain_refine;\n'
                'int (*measure)(cvs_handle, const int32_t*, int, const cvs_chain*, int, const float*, const float*, cvs_chain_measure*, int)'
                ' = cvs_chain_measures;\n'
                'int main() { return refine == 0 || measure == 0; }\n')
    subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), src], check=True)


def test_libraries_export_and_bind():
    import cvsteer_amd
    from cvsteer_amd import _lib as L
    assert L.SIGNATURES["cvs_chain_refine"] == (C.c_int, [C.c_void_p, L._PP, L._PP, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int])
    assert L.SIGNATURES["cvs_chain_measures"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                            C.c_void_p, C.c_int])
    assert C.sizeof(L.ChainMeasure) == 40 == M.MEASURE_DTYPE.itemsize
    hip = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "cvsteer_amd", "libcvsteer_hip.so")], text=True)
    assert re.search(r" T cvs_chain_refine$", hip, re.M) and re.search(r" T cvs_chain_measures$", hip, re.M)
    so = os.path.join(ROOT, "cvsteer_amd", "libcvsteer.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cvsteer_amd", "facade"), "-s"])
    syms = subprocess.check_output(["nm", "-DC", "--defined-only", so], text=True)
    for cls in ("SteerableFiltersG2", "SteerableFiltersG4"):
        assert re.search(r" T fa::%s::refineContours\(fa::Mat1f const&, std::vector<std::vector<fa::Point," % cls, syms), cls
    for cls in (cvsteer_amd.SteerableFiltersG2, cvsteer_amd.SteerableFiltersG4):
        assert all(callable(getattr(cls, name, None)) for name in ("chain_refine", "chain_measures", "contour_edgels"))
        assert cls.MEASURE_DTYPE == M.MEASURE_DTYPE
        assert [(n, cls.MEASURE_DTYPE.fields[n][1]) for n in cls.MEASURE_DTYPE.names] == \
               [(n, getattr(L.ChainMeasure, n).offset) for n, _ in L.ChainMeasure._fields_]


def test_null_handle():
    from cvsteer_amd import _lib as L
    pts = np.zeros((3, 2), np.int32)
    tab = np.array([[0, 3, 0, 0]], np.int32)
    img = np.zeros((4, 4), F32)
    plane = L.Plane(img.ctypes.data, 4, 4, 16, L.MEM_HOST)
    xy, st, rec = np.full((3, 2), -9, F32), np.full((3,), -9, F32), np.full((1, 10), -9, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert L.lib().cvs_chain_refine(None, C.byref(plane), C.byref(plane), p(pts), 3, p(xy), p(st), L.MEM_HOST) == L.E_BADARG
    assert L.lib().cvs_chain_measures(None, p(pts), 3, p(tab), 1, p(xy), p(st), p(rec), L.MEM_HOST) == L.E_BADARG
    assert (xy == -9).all() and (st == -9).all() and (rec == -9).all()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_refine_kernels_use_no_scratch(tmp_path):
    path = os.path.join(str(tmp_path), "cvs_kernels_refine.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    "-I" + SRC, "-S", "--cuda-device-only", os.path.join(SRC, "cvs_kernels_refine.hip"), "-o", path], check=True,
                   stderr=subprocess.DEVNULL)
    text = open(path).read()
    scratch = {}
    for blk in text.split("  - .agpr_count:")[1:]:
        nm = re.search(r"\.name:\s+(\S+)", blk)
        ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        if nm and ps:
            scratch[nm.group(1)] = int(ps.group(1))
    for stem in ("k_chain_refine", "k_measure_wave", "k_measure_block"):
        assert any(stem in n for n in scratch), (stem, sorted(scratch))
    assert len(scratch) == 3 and all(v == 0 for v in scratch.values()), scratch
    # the point and the position travel as one 8-byte access each
    body = text[text.index("k_chain_refine"):]
    body = body[:body.index(".Lfunc_end")]
    assert "global_load_dwordx2" in body and "global_store_dwordx2" in body


# ---- the refinement model against the contract's own consequences ----
def _random_case(seed, shape=(33, 65)):
    rng = np.random.default_rng(seed)
    m = rng.random(shape, dtype=F32)
    theta = (np.pi - 2 * np.pi * rng.random(shape)).astype(F32)               # (-pi, pi]
    return m, theta


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_float32_samples_are_those_of_the_thinning_model():
    for seed in range(3):
        m, theta = _random_case(seed)
        c, s = M.directions(theta)
        P = M.refine_map(m, c, s)
        thin, vb, vf = NM.nonmax_parts(m, c, s)
        assert np.array_equal(_bits(vb), _bits(P["vb"])) and np.array_equal(_bits(vf), _bits(P["vf"]))
        assert np.array_equal(P["keep"], thin > 0)                           # the keep test is that of cvs_nonmax (m > 0 here)


def test_offset_is_at_most_half_a_pixel_everywhere():
    tiny, huge = np.float32(1e-38), np.float32(1e30)
    n = 0
    for seed in range(4):
        m, theta = _random_case(seed)
        rng = np.random.default_rng(100 + seed)
        m = m * rng.choice(np.array([1.0, 1.0, tiny, huge, 1e-45], F32), m.shape)   # plateaus of denormals, large steps
        m[rng.random(m.shape) < 0.05] = 0.0
        if seed == 3:
            m = np.round(m * 4) / 4                                          # many exact ties: a == b, a == 0
        for th in (theta, np.zeros_like(theta), np.full_like(theta, np.pi / 4), np.full_like(theta, -3 * np.pi / 4)):
            P = M.refine_map(m.astype(F32), *M.directions(th))
            assert P["t"].dtype == F32 and np.isfinite(P["t"]).all()
            assert float(np.abs(P["t"]).max()) <= 0.5
            y, x = np.mgrid[0:m.shape[0], 0:m.shape[1]]
            assert float(np.abs(P["xs"] - x).max()) <= 0.5 and float(np.abs(P["ys"] - y).max()) <= 0.5
            n += int(P["keep"].sum())
    assert n > 3000


def test_no_offset_and_the_sample_itself_where_the_keep_test_fails():
    m, theta = _random_case(7)
    m[5, 9] = np.nan                                                          # NaN in m: that pixel and its eight neighbours see it
    m[20, 30] = np.nan
    theta[11, 40] = np.nan                                                    # NaN in theta
    P = M.refine_map(m, *M.directions(theta))
    fail = ~P["keep"]
    assert fail.sum() > 500 and P["keep"].sum() > 100
    assert not P["t"][fail].any() and not np.signbit(P["t"][fail]).any()      # t is +0.0
    assert np.array_equal(_bits(P["strength"][fail]), _bits(m[fail]))         # m bit for bit, the NaN included
    assert fail[5, 9] and fail[20, 30] and fail[11, 40]
    assert np.isnan(P["strength"][5, 9]) and P["strength"][11, 40] == m[11, 40]
    # a NaN neighbour: wherever it enters a sample with a weight that is not zero the test fails; the pixel keeps its own value
    near = [(r, c) for r in (4, 5, 6) for c in (8, 9, 10) if (r, c) != (5, 9)]
    hit = [(r, c) for r, c in near if np.isnan(P["vb"][r, c]) or np.isnan(P["vf"][r, c])]
    assert len(hit) >= 2
    for r, c in hit:
        assert fail[r, c] and P["t"][r, c] == 0 and _bits(P["strength"][r, c]) == _bits(m[r, c])
    # where the test holds the strength is the vertex of the parabola: never below the sample
    k = P["keep"]
    assert (P["strength"][k] >= m[k]).all()
    # ... and the position is the pixel centre, a NaN theta (whose weight is NaN) included
    y, x = np.mgrid[0:m.shape[0], 0:m.shape[1]]
    assert np.array_equal(_bits(P["xs"][fail]), _bits(x[fail])) and np.array_equal(_bits(P["ys"][fail]), _bits(y[fail]))
    assert P["xs"][11, 40] == 40 and P["ys"][11, 40] == 11
    xy, st = M.gather(P, [(9, 5), (-1, 0), (0, 33), (65, 0), (64, 32)])
    assert np.isnan(xy[1:4]).all() and np.isnan(st[1:4]).all() and np.isfinite(xy[4]).all() and np.isnan(st[0])


def test_ridges_are_located_to_a_tenth_of_a_pixel():
    """48 x 48 ridges exp(-d^2 / 4.5) + 0.002 noise through (24.3, 24.1), analytic theta; the points NMS keeps with m > 0.5, 6 px from the
    border.  The refined points must lie within 0.1 px of the line (the model's own worst figure is 0.064 px, at 133 degrees); the pixel
    centres of the same points lie more than 0.5 px off at every oblique angle (worst 0.69 px at 133 degrees) but one: at 135 degrees the
    centres sit on the two lattice diagonals next to the line, 0.4 / sqrt(2) and 0.6 / sqrt(2) px away -- a fact of the lattice, whatever
    the code does -- so there the figure required is 0.6 / sqrt(2) itself."""
    worst_ref = worst_pix = 0.0
    for deg in M.GEOMETRY_ANGLES:
        img, theta, dist = M.ridge(48, deg)
        c, s = M.directions(theta)
        P = M.refine_map(img, c, s)
        thin = NM.nonmax_parts(img, c, s)[0]
        sel = thin > 0.5
        sel[:6], sel[-6:], sel[:, :6], sel[:, -6:] = False, False, False, False
        assert sel.sum() >= 30 and P["keep"][sel].all()
        y, x = np.nonzero(sel)
        d_ref = float(np.abs(dist(P["xs"][sel], P["ys"][sel])).max())
        d_pix = float(np.abs(dist(x, y)).max())
        print("ridge %6.1f deg: %3d points, refined %.4f px, pixel centres %.4f px" % (deg, sel.sum(), d_ref, d_pix))
        assert d_ref <= 0.1, (deg, d_ref)
        if deg == 135.0:
            assert abs(d_pix - 0.6 / np.sqrt(2)) < 1e-6 and d_pix > 6 * d_ref
        elif deg not in (0.0, 90.0):
            assert d_pix > 0.5, (deg, d_pix)
        # the float64 formulas agree with the float32 ones to rounding
        P64 = M.refine_map(img, np.float64(c), np.float64(s), np.float64)
        assert float(np.abs(P64["xs"][sel] - P["xs"][sel]).max()) < 1e-5 and float(np.abs(P64["ys"][sel] - P["ys"][sel]).max()) < 1e-5
        worst_ref, worst_pix = max(worst_ref, d_ref), max(worst_pix, d_pix)
    assert worst_ref < 0.07 and worst_pix > 0.68


# ---- the measures model against a second computation ----
def _brute(points, chains, strength, xy):
    out = []
    for start, n, flags, _ in chains.tolist():
        p = points[start:start + n].astype(np.int64)
        q = np.roll(p, -1, axis=0) if flags & CM.CLOSED else p[1:]
        d = np.abs(q - p[:len(q)])
        axial = int(((d[:, 0] + d[:, 1]) == 1).sum())
        diagonal = int(((d[:, 0] == 1) & (d[:, 1] == 1)).sum())
        g = (points if xy is None else xy)[start:start + n].astype(np.float64)
        e = (np.roll(g, -1, axis=0) if flags & CM.CLOSED else g[1:]) - g[:len(q)]
        length = float(np.sqrt(e[:, 0] ** 2 + e[:, 1] ** 2).sum())
        rec = dict(axial=axial, diagonal=diagonal, other=len(q) - axial - diagonal, length=length)
        if strength is not None:
            v = strength[start:start + n]
            ok = ~np.isnan(v)
            rec.update(sum=float(v.astype(np.float64).sum()), peak=float(v[ok].max()) if ok.any() else -np.inf,
                       weakest=float(v[ok].min()) if ok.any() else np.inf,
                       peak_index=start + int(np.nonzero(ok & (v == v[ok].max()))[0][0]) if ok.any() else -1)
        else:
            rec.update(sum=0.0, peak=-np.inf, weakest=np.inf, peak_index=-1)
        out.append(rec)
    return out


def test_measures_model_on_the_chains_of_random_masks():
    rng = np.random.default_rng(5)
    n_chains = n_closed = 0
    for density in (0.15, 0.3, 0.5):
        mask = (rng.random((33, 65)) < density).astype(F32)
        if density == 0.15:
            mask[10:14, 20:24] = 0
            mask[10, 20:24] = mask[13, 20:24] = mask[10:14, 20] = mask[10:14, 23] = 1   # a ring: one closed chain
            mask[9, 19:25] = mask[14, 19:25] = mask[9:15, 19] = mask[9:15, 24] = 0
        points, chains = CM.chains(mask)
        strength = rng.standard_normal(len(points)).astype(F32)
        strength[rng.random(len(points)) < 0.05] = np.nan
        xy = (points + rng.uniform(-0.5, 0.5, points.shape)).astype(F32)
        for st, sub in ((strength, xy), (None, None), (strength, None), (None, xy)):
            got = M.measures(points, chains, st, sub)
            want = _brute(points, chains, st, sub)
            assert (got["other"] == 0).all()                                   # chains of cvs_contour_chains step to 8-neighbours only
            for g, w, (start, n, flags, _) in zip(got, want, chains.tolist()):
                assert (g["axial"], g["diagonal"], g["other"], g["peak_index"]) == (w["axial"], w["diagonal"], w["other"], w["peak_index"])
                assert g["axial"] + g["diagonal"] == n - 1 + (flags & CM.CLOSED)
                assert g["peak"] == np.float32(w["peak"]) and g["weakest"] == np.float32(w["weakest"])
                assert (np.isnan(g["sum"]) and np.isnan(w["sum"])) or abs(g["sum"] - w["sum"]) <= 1e-12 * max(1.0, n)
                assert abs(g["length"] - w["length"]) <= 1e-12 * max(1.0, n)
                if sub is None:
                    assert abs(g["length"] - (g["axial"] + g["diagonal"] * np.sqrt(2.0))) <= 1e-12 * max(1.0, n)
        n_chains += len(chains)
        n_closed += int((chains[:, 2] & CM.CLOSED).astype(bool).sum())
    assert n_chains >= 150 and n_closed >= 1


def test_measures_model_hand_cases():
    pts = np.int32([[5, 7], [1, 1], [2, 2], [2, 3], [9, 9]])
    tab = np.int32([[0, 1, 0, 0], [1, 3, 0, 0], [1, 3, CM.CLOSED, 0], [3, 2, 0, 0], [4, 2, 0, 0], [0, 1, CM.CLOSED, 0]])
    st = np.float32([2.0, -1.0, np.nan, 3.0, 3.0])
    got = M.measures(pts, tab, st)
    assert got[0].tolist() == (0, 0, 0, 0, 2.0, 2.0, 2.0, 0.0)                 # an isolated point
    assert list(got[1].tolist()[:4]) == [1, 1, 0, 3] and np.isnan(got[1]["sum"]) and got[1]["weakest"] == -1.0
    assert abs(got[1]["length"] - (1 + np.sqrt(2.0))) < 1e-15
    assert (got[2]["axial"], got[2]["diagonal"], got[2]["other"]) == (1, 1, 1)  # the closing step (2, 3) -> (1, 1) is neither
    assert (got[3]["peak_index"], got[3]["peak"], got[3]["other"]) == (3, 3.0, 1)   # the first of two equal peaks
    assert got[4].tolist() == (0, 0, 0, -1, 0.0, 0.0, 0.0, 0.0)                # an entry beyond the points: the empty record
    assert (got[5]["other"], got[5]["length"]) == (1, 0.0)                     # a closed chain of one point steps onto itself
    none = M.measures(pts, tab[:2])
    assert list(none[1].tolist()[3:7]) == [-1, -np.inf, np.inf, 0.0]
