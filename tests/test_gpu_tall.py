"""GPU test (-m gpu): tall images, one workgroup row past 65535 and past 65536 for every launcher whose grid.y follows the image height
(cvsteer_amd/csrc/cvs_grid.h; tests/test_grid_plan_cpu.py sweeps the same arithmetic on the CPU).  Each case names the launcher it
drives and takes its row count from the constants in the sources: 65537 units of that launcher's tiling.  Every call goes through the
Python surface, which raises on any status but CVS_OK -- no case may end in CVS_E_HIP -- and every result is held to the reference the
small-shape suites use for the same call: the float64 oracle within TOL for filtered planes, bit identity between launch plans, the
numpy / scipy models byte for byte for the contour calls."""
import os
import re

import numpy as np
import pytest
import torch

import chains_model
import components_model
import contour_model
import cvsteer_amd as cv
import link_model
from cvsteer_amd import _lib as L
from test_gpu_bench_instances import _oracle_basis_rows
from test_gpu_components import _check_table
from test_gpu_contours import _check_nms, _random_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
TOL = 1e-5          # tests/test_gpu_parity.py: basis planes on [0, 1) inputs against the f64-accumulated oracle
UNITS = 65537       # one past either candidate limit of grid.y


def _src(name):
    return open(os.path.join(ROOT, "cvsteer_amd", "csrc", name)).read()


def _const(text, name):
    return int(re.search(r"\b%s = (\d+)" % name, text).group(1))


CC_TILE_H = _const(_src("cvs_components.h"), "kCcTileH")
CH_ROWS = _const(_src("cvs_kernels_chains.hip"), "kChRows")
HYST_TILE_H = _const(_src("cvs_kernels_contour.hip"), "kHystTileH")
NMS_STRIP_MAX = int(re.search(r"strip > (\d+) \? \1 : strip", _src("cvs_grid.h")).group(1))   # the thinning strip clamp
# k_pyr_down: four waves of two output rows per workgroup = 16 source rows (pyr_down_group_count)
assert "(((rows + 1) / 2 + 1) / 2 + 3) / 4" in _src("cvs_grid.h")
PYR_SRC_ROWS = 16
assert CC_TILE_H == CH_ROWS == HYST_TILE_H, "one row count serves the three 32-row tilings"
ROWS_GENERIC = UNITS                              # 65,537: one row per workgroup row
ROWS_STRIP10 = 10 * (UNITS - 1) + 1               # 655,361: 65,537 ten-row strips
ROWS_PYR = PYR_SRC_ROWS * (UNITS - 1) + 1         # 1,048,577
ROWS_TILE = CC_TILE_H * (UNITS - 1) + 1           # 2,097,153: the last tile is one row high
ROWS_NMS = NMS_STRIP_MAX * (UNITS - 1) + 1        # 4,194,305


def _image(rows, cols, seed):
    return torch.rand((rows, cols), generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV)


def _state_planes(f, nb):
    return [f.basis(p) for p in range(nb)] + list(f.coefficients()) + [f.getDominantOrientationAngle(), f.getDominantOrientationStrength()]


def _bands(rows):
    mid = rows // 2 - 12
    return ((0, 24), (mid, mid + 24), (rows - 24, rows))


def _oracle_rows(ora, kind, img, lo, hi):
    """_oracle_basis_rows for either bank: rows [lo, hi) of the whole-image filter, from a band with W rows of context"""
    if kind == 2:
        return _oracle_basis_rows(ora, img, lo, hi)
    n, w = img.shape[0], 6
    a, b = max(0, lo - w), min(n, hi + w)
    return ora.basis(4, img[a:b], 6, 0.5, f64=True)[:, lo - a:lo - a + (hi - lo)]


# ----------------------------------------------------------------------------- generic path: launch_generic, grid.y = rows
@pytest.mark.parametrize("kind,w,s,cols", [(2, 4, 0.67, 3), (2, 6, 0.5, 9), (4, 6, 0.5, 5)], ids=["g2_default_3_cols", "g2_w6", "g4_default_5_cols"])
def test_generic_path_65537_rows(ora, kind, w, s, cols):
    """k_rowpass_generic / k_colpass_generic (every non-default width, and default taps on images narrower than W + 1 columns) and the
    per-pixel launches behind them, at 65,537 rows: all basis planes of the whole image against the f64 oracle as
    test_generic_width_path does, and full setup plus pipeline against the stepwise calls as test_generic_width_full_surface does."""
    img = _image(ROWS_GENERIC, cols, seed=11 * cols + w)
    host = img.cpu().numpy()
    nb = 7 if kind == 2 else 11
    new = (lambda: cv.SteerableFiltersG2(None, w, s)) if kind == 2 else (lambda: cv.SteerableFiltersG4(None, w, s, extensions=True))
    f = new()
    f.setup(img, flags=cv.SETUP_FULL)
    got = np.stack([f.basis(p).cpu().numpy() for p in range(nb)])
    err = float(np.abs(got - ora.basis(kind, host, w, s, f64=True)).max())
    print("generic %dx%d kind %d width %d: max |basis - f64 oracle| %.3g" % (ROWS_GENERIC, cols, kind, w, err))
    assert err <= TOL
    g0, h0, e0, m0, p0 = f.steer(None, full=True)
    ed, dk, br = f.find(m0, p0)
    fused = new().pipeline(img)
    for a, b in zip((g0, h0, e0, m0, p0, ed, dk, br), fused):
        assert torch.equal(a, b)
    g1, h1 = new().setup_steer(img, 0.3)
    g2, h2 = f.steer(0.3)
    assert torch.equal(g1, g2) and torch.equal(h1, h2)
    if kind == 2:   # the oracle's own orientation and steer on the planes the GPU made, on the three bands
        for lo, hi in _bands(ROWS_GENERIC):
            o1, o2, o3, oth, ost = ora.g2_orientation(got[:, lo:hi])
            og, oh = ora.g2_steer_scalar(got[:, lo:hi], 0.3)
            assert np.abs(g2[lo:hi].cpu().numpy() - og).max() <= 1e-6 and np.abs(h2[lo:hi].cpu().numpy() - oh).max() <= 1e-6
            assert np.abs(f.getDominantOrientationStrength()[lo:hi].cpu().numpy() - ost).max() <= 1e-6


# ----------------------------------------------------------------------------- strip kernels, plain order: plan_strips, grid.y = strips
def _run_pipeline(kind, img, order, strip, calls):
    """`calls` pipeline runs on one handle with the order / strip height forced (None: left alone); the outputs and state planes of the
    last run (all runs agree), and the (block_order, strip_rows) launch_info reported after each"""
    f = cv.SteerableFiltersG2(None) if kind == 2 else cv.SteerableFiltersG4(None, extensions=True)
    if order is not None:
        f.set_option(L.OPT_BLOCK_ORDER, order)
    if strip:
        f.set_strip_rows(strip)
    ran, first = [], None
    for _ in range(calls):
        outs = f.pipeline(img)
        torch.cuda.synchronize()
        info = f.launch_info()
        ran.append((info["block_order"], info["strip_rows"]))
        planes = list(outs) + _state_planes(f, 7 if kind == 2 else 11)
        if first is None:
            first = planes
        else:
            for a, b in zip(planes, first):
                assert torch.equal(a, b)
    return f, first, ran


def _check_basis_bands(ora, kind, f, img):
    host = img.cpu().numpy()
    nb = 7 if kind == 2 else 11
    state = [f.basis(p) for p in range(nb)]
    for lo, hi in _bands(img.shape[0]):
        b = np.stack([s[lo:hi].cpu().numpy() for s in state])
        assert np.abs(b - _oracle_rows(ora, kind, host, lo, hi)).max() <= TOL, (lo, hi)


@pytest.mark.parametrize("kind,cols", [(2, 5), (4, 7)], ids=["g2", "g4_pair"])
def test_plain_order_one_row_strips_65537_rows(ora, kind, cols):
    """k_basis / k_basis_lit (G2) and k_basis_pair (G4) in the plain order with CVS_OPT_STRIP_ROWS = 1 at 65,537 rows: 65,537 strips.  Every
    state plane and the eight pipeline outputs bit-identical to a default handle's, the basis planes against the oracle on the top,
    middle and bottom 24 rows, and launch_info says the forced height and order ran."""
    img = _image(ROWS_GENERIC, cols, seed=500 + cols)
    f, forced, ran = _run_pipeline(kind, img, L.ORDER_PLAIN, 1, calls=3)
    assert ran == [(L.ORDER_PLAIN, 1)] * 3, ran
    _, default, _ = _run_pipeline(kind, img, None, 0, calls=1)
    for k, (a, b) in enumerate(zip(forced, default)):
        assert torch.equal(a, b), k
    _check_basis_bands(ora, kind, f, img)


def test_plain_order_default_strips_655361_rows(ora):
    """G2 at 655,361 x 5 in the plain order with the default ten-row strips (65,537 of them), and with the tuner's seven-row challenger
    pinned (93,623 strips; three calls never leave the default's turn of at least 20, so the challenger gets a leg of its own):
    bit-identical to each other, to the dynamic tail and to the XCD-column order, whose grids are one-dimensional, with the three
    oracle bands."""
    img = _image(ROWS_STRIP10, 5, seed=77)
    f, plain, ran = _run_pipeline(2, img, L.ORDER_PLAIN, 0, calls=3)
    assert ran == [(L.ORDER_PLAIN, 10)] * 3, ran
    assert (ROWS_STRIP10 + 9) // 10 == UNITS
    for order, strip in ((L.ORDER_PLAIN, 7), (L.ORDER_DYNAMIC_TAIL, 0), (L.ORDER_XCD_COLUMNS, 0)):
        _, other, ran_o = _run_pipeline(2, img, order, strip, calls=1)
        assert ran_o[0][0] == order and (not strip or ran_o[0][1] == strip), ran_o
        for k, (a, b) in enumerate(zip(plain, other)):
            assert torch.equal(a, b), (order, strip, k)
        del other
    _check_basis_bands(ora, 2, f, img)


def test_8bit_pipeline_stays_one_launch_through_the_tuners_turns():
    """The 8-bit three-maps pipeline exists as ONE fused launch only, judged so with the default's ten-row strips before the tuner is
    asked.  At 500,000 x 8 ten-row strips fit one plain grid (50,000 strips) and the tuner's seven-row challenger does not (71,429): the
    challenger must pass its turn, never turn the call into CVS_E_HIP.  250 calls run well past the default's first turn (20 to 100
    calls); every call returns CVS_OK (the surface raises otherwise) and the same bytes, which are those of a handle with the tuner
    off and of the composed route (f32 maps through normalize_u8)."""
    rows, cols = 500000, 8
    assert 65535 * 7 < rows <= 65535 * 10
    img = _image(rows, cols, seed=8)
    f = cv.SteerableFiltersG2(None)
    f.set_persist(False)
    outs = [None] * 5 + [torch.empty((rows, cols), dtype=torch.uint8, device=DEV) for _ in range(3)]
    first, strips = None, set()
    for call in range(250):
        f.pipeline(img, out=outs)
        info = f.launch_info()
        strips.add((info["block_order"], info["strip_rows"], info["u8_out"]))
        if first is None:
            assert info["u8_out"] == 2, info   # the default's plan IS the fused launch (min / max reduced in it)
            first = [o.clone() for o in outs[5:]]
        elif call % 10 == 0 or call > 240:
            for a, b in zip(outs[5:], first):
                assert torch.equal(a, b), call
    torch.cuda.synchronize()
    print("8-bit pipeline %dx%d: (order, strip, u8_out) seen %s" % (rows, cols, sorted(strips)))
    assert all(s * 65535 >= rows for o, s, u in strips if u and o == L.ORDER_PLAIN), strips   # a fused launch was never one that bands
    quiet = cv.SteerableFiltersG2(None)
    quiet.set_option(L.OPT_AUTOTUNE, 0)
    quiet.set_persist(False)
    ref = quiet.pipeline(img, out=[None] * 5 + [torch.empty((rows, cols), dtype=torch.uint8, device=DEV) for _ in range(3)])
    plain = cv.SteerableFiltersG2(None)
    maps = plain.pipeline(img)[5:]
    for a, b, m in zip(first, ref[5:], maps):
        assert torch.equal(a, b)
        assert torch.equal(a, plain.normalize_u8(m))


def test_batch_of_tall_frames_equals_frame_by_frame():
    """a batch launch is never banded (frames lie on grid.z): frames of 65,537 rows, which one-row strips would not fit, go frame by frame
    through the single-image path (strip_batch_fits) -- every plane bit-identical to pipeline() per frame, with and without forced strips"""
    frames = torch.rand((3, ROWS_GENERIC, 5), generator=torch.Generator(device=DEV).manual_seed(9), device=DEV)
    for order, strip in ((None, 0), (L.ORDER_PLAIN, 1)):
        eng = cv.SteerableFiltersG2(None)
        if order is not None:
            eng.set_option(L.OPT_BLOCK_ORDER, order)
            eng.set_strip_rows(strip)
        out = eng.pipeline_batch(frames)
        for i in range(3):
            ref = cv.SteerableFiltersG2(None).pipeline(frames[i])
            for k in range(8):
                assert torch.equal(out[i, k], ref[k]), (order, i, k)


# ----------------------------------------------------------------------------- launch_pyr_down: grid.y = groups of 16 source rows
@pytest.mark.parametrize("cols", [2, 5])
def test_pyr_down_and_setup_pyr_1048577_rows(ora, cols):
    """cvs_pyr_down and cvs_setup_pyr at 1,048,577 source rows, 65,537 groups of k_pyr_down.  Which kernel a leg reaches:
      2 columns (under the strip march's W + 1 = 5): pyrDown and setup_pyr's composed route both run k_pyr_down and its stride loop;
      5 columns: pyrDown takes the strip march (46-row strips, 22,796 of them -- NOT k_pyr_down) and setup_pyr the fused launch that
      emits the level, which the plain order bands at this height; k_pyr_down is not reached in this leg.
    The oracle's pyr_down bit for bit, as test_pyr_down_matches_oracle asks; cvs_setup_pyr equals cvs_setup followed by cvs_pyr_down."""
    img = _image(ROWS_PYR, cols, seed=31 + cols)
    f = cv.SteerableFiltersG2(None)
    down = f.pyrDown(img)
    assert tuple(down.shape) == ((ROWS_PYR + 1) // 2, (cols + 1) // 2)
    assert np.array_equal(down.cpu().numpy(), ora.pyr_down(img.cpu().numpy()))
    g = cv.SteerableFiltersG2(None)
    nxt = g.setup_pyr(img, flags=cv.SETUP_BASIS)
    assert torch.equal(nxt, down)
    ref = cv.SteerableFiltersG2(None)
    ref.setup(img, flags=cv.SETUP_BASIS)
    for p in range(7):
        assert torch.equal(g.basis(p), ref.basis(p)), p


# ----------------------------------------------------------------------------- 32-row tiles: 2,097,153 rows
@pytest.fixture(scope="module")
def tall5():
    """one handle of 2,097,153 x 5 (five columns: its own setup takes the strip path) with the two masks, the map and their models"""
    rows, cols = ROWS_TILE, 5
    f = cv.SteerableFiltersG2(None)
    f.setup(torch.zeros((rows, cols), device=DEV), flags=cv.SETUP_BASIS)
    rng = np.random.default_rng(2097153)
    dense = (rng.random((rows, cols)) < 0.5).astype(np.float32)
    banded = np.zeros((rows, cols), np.float32)
    mid = rows // 2
    for lo, hi in ((0, 40), (mid - 20, mid + 20), (rows - 70, rows)):   # the last band crosses into the one-row tile
        banded[lo:hi] = rng.random((hi - lo, cols)) < 0.6
    vmap = rng.random((rows, cols), dtype=np.float32)
    return {"f": f, "dense": dense, "banded": banded, "map": vmap}


@pytest.mark.parametrize("which", ["dense", "banded"])
def test_label_prune_stats_points_2097153_rows(tall5, which):
    """k_cc_tiles at 65,537 tile rows behind cvs_label, cvs_contour_prune, cvs_component_stats and cvs_contour_points: exact"""
    f, mask = tall5["f"], tall5[which]
    dm = torch.from_numpy(mask).to(DEV)
    want, wn = components_model.label(mask)
    lab, n = f.label(dm)
    assert n == wn
    assert torch.equal(lab, torch.from_numpy(want).to(DEV))
    weight = tall5["map"]
    pr, kept = f.prune(dm, 3, weight=torch.from_numpy(weight).to(DEV), min_peak=0.5, return_kept=True)
    wp, wk = components_model.prune(mask, 3, weight, 0.5)
    assert kept == wk and torch.equal(pr, torch.from_numpy(wp).to(DEV))
    _check_table(f.component_stats(lab, n, torch.from_numpy(weight).to(DEV)), components_model.stats(want, wn, weight))
    pts = f.contour_points(lab)
    assert np.array_equal(pts.cpu().numpy(), components_model.points(want))


def test_label_single_column_2097153_rows():
    """the single-column corner: 2,097,153 x 1, whose setup takes the generic path (grid.y = rows before the cap)"""
    rows = ROWS_TILE
    f = cv.SteerableFiltersG2(None)
    f.setup(torch.zeros((rows, 1), device=DEV), flags=cv.SETUP_BASIS)
    mask = (np.random.default_rng(5).random((rows, 1)) < 0.5).astype(np.float32)
    want, wn = components_model.label(mask)
    lab, n = f.label(torch.from_numpy(mask).to(DEV))
    assert n == wn and torch.equal(lab, torch.from_numpy(want).to(DEV))


def test_hysteresis_2097153_rows(tall5):
    """k_hyst_propagate at 65,537 tile rows: a uniform [0, 1) map at 0.55 / 0.8 against the model, byte for byte"""
    f, v = tall5["f"], tall5["map"]
    got, passes = f.hysteresis(torch.from_numpy(v).to(DEV), 0.55, 0.8, return_passes=True)
    print("hysteresis %s: %d passes" % (v.shape, passes))
    assert torch.equal(got, torch.from_numpy(contour_model.hysteresis(v, 0.55, 0.8)).to(DEV))


def test_contour_chains_2097153_rows(tall5):
    """k_ch_links (65,537 bands of 32 rows) and k_cc_tiles behind cvs_contour_chains, on the banded mask: exact"""
    f, mask = tall5["f"], tall5["banded"]
    pts, table = f.contour_chains(torch.from_numpy(mask).to(DEV))
    want_p, want_t = chains_model.chains(mask)
    assert tuple(pts.shape) == want_p.shape and tuple(table.shape) == want_t.shape
    assert np.array_equal(table.cpu().numpy(), want_t) and np.array_equal(pts.cpu().numpy(), want_p)


def test_link_2097153_rows(tall5):
    """k_link_tiles at 65,537 tile rows: cvs_link accepts what cvs_label accepts (CVS_OK; the row refusal is gone) and equals the model,
    byte for byte and count for count"""
    f, v = tall5["f"], tall5["map"]
    got, kept = f.link(torch.from_numpy(v).to(DEV), 0.55, 0.8, min_area=3, return_kept=True)
    want, wk = link_model.link(v, 0.55, 0.8, 3)
    assert int(kept) == wk and torch.equal(got, torch.from_numpy(want).to(DEV))


# ----------------------------------------------------------------------------- thinning: nonmax_grid, 64-row strips
@pytest.mark.parametrize("cols", [1, 5])
def test_nonmax_4194305_rows(cols):
    """k_nonmax at 4,194,305 rows, where 64-row strips would need 65,537 of them: identical to the model at every decided pixel, the
    undecided share under _check_nms's 1e-3 cap (the model alone leaves 23 of 4,194,241 x 1 and 51 of 4,194,241 x 2 pixels undecided)"""
    rows = ROWS_NMS
    maps, th = _random_case(rows, cols, seed=rows + cols, sprinkle=False)
    f = cv.SteerableFiltersG2(None)
    f.setup(torch.zeros((rows, cols), device=DEV), flags=cv.SETUP_BASIS)
    got = f.nonmax(torch.from_numpy(maps[0]).to(DEV), theta=torch.from_numpy(th).to(DEV))
    _check_nms(got, maps[0], th)


# ----------------------------------------------------------------------------- the device's own figures ("Grid bounds")
def test_device_grid_limits_admit_the_bound():
    """hipDeviceAttributeMaxGridDimX / Y / Z of the device, read from the loaded HIP runtime: kGridMaxYZ = 65535 and x < 2^24 must lie
    inside whatever it reports"""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    dims = []
    for attr in (29, 30, 31):   # hipDeviceAttributeMaxGridDimX, ..Y, ..Z (hip_runtime_api.h)
        v = C.c_int(0)
        assert hip.hipDeviceGetAttribute(C.byref(v), attr, 0) == 0
        dims.append(v.value)
    print("hipDeviceAttributeMaxGridDim X / Y / Z: %d / %d / %d" % tuple(dims))
    assert dims[0] >= (1 << 24) - 1 and dims[1] >= 65535 and dims[2] >= 65535
