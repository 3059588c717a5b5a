"""CPU test: the grid arithmetic of every launcher whose grid.y or grid.z follows the image height (cvsteer_amd/csrc/cvs_grid.h).
tests/cpp/grid_plan.cpp, a stand-alone program with no device and no HIP header in it, is built with g++ under AddressSanitizer and
UndefinedBehaviorSanitizer the way test_sanitizers_cpu.py builds its harnesses, and run twice: on the functions of cvs_grid.h, which
must hold every requirement (y, z <= 65535, x * 256 < 2^32, every row / tile row / strip covered exactly once, the grids of the timed
shapes unchanged), and on the formulas the launchers had before, which must break them in every launcher family."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cvsteer_amd", "csrc")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
FAMILIES = ("generic_grid", "tile_grid", "pyr_down_grid", "nonmax_grid", "strip plan")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("grid_plan") / "grid_plan")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SAN + ["-Icvsteer_amd/csrc", "tests/cpp/grid_plan.cpp", "-o", out],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def _run(exe, *args):
    r = subprocess.run([exe] + list(args), cwd=ROOT, capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-1500:]
    return r


def _broken(stdout):
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^([a-z_ ]+): (\d+) broken$", stdout, re.M)}


def test_every_grid_holds_the_bounds_and_covers_every_row_once(exe):
    r = _run(exe)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "grid plan holds" in r.stdout and "FAIL" not in r.stdout
    broken = _broken(r.stdout)
    assert set(FAMILIES) | {"timed"} <= set(broken) and not any(broken.values()), broken
    assert int(re.search(r"(\d+) grids checked", r.stdout).group(1)) > 100000   # the sweep ran


def test_the_formulas_the_launchers_had_before_break_the_bounds(exe):
    r = _run(exe, "parent")
    assert r.returncode == 1, (r.returncode, r.stdout[-2000:])
    broken = _broken(r.stdout)
    for fam in FAMILIES:   # each family passed 65535 rows of workgroups somewhere in the sweep
        assert broken.get(fam, 0) > 0, (fam, broken)
    for shape in ("generic_grid 65537x3", "strip plan 65537x5 strip 1 order 0", "pyr_down_grid 1048577x2", "2097153x5 x1: grid.y > 65535"):
        assert shape in r.stdout, shape


def test_the_launchers_take_their_grids_from_the_header():
    """Every launcher of the table calls the header's functions, the program's tile constants are the sources', and the header has no HIP
    type in it (the program above includes it with nothing else).  That the grids are right is held by the sweep above and, for the
    lifted cvs_link refusal, by tests/test_gpu_tall.py."""
    def src(name):
        return open(os.path.join(CSRC, name)).read()

    hdr = src("cvs_grid.h")
    assert "dim3" not in hdr and "#include" not in hdr
    uses = {"cvs_kernels_basis.hip": ("generic_grid(", "strip_grid(", "strip_band_cap(", "strip_band_rows("),
            "cvs_kernels_point.hip": ("pyr_down_grid(", "pyr_down_group_count("),
            "cvs_kernels_components.hip": ("tile_grid(", "tile_row_count("),
            "cvs_kernels_link.hip": ("tile_grid(", "tile_row_count("),
            "cvs_kernels_chains.hip": ("tile_grid(", "tile_row_count("),
            "cvs_kernels_chains_batch.hip": ("tile_grid(", "tile_row_count("),
            "cvs_kernels_contour.hip": ("tile_grid(", "tile_row_count(", "nonmax_grid(b.rows"),
            "cvs_tune.cpp": ("strip_one_launch(",), "cvs_pipeline.cpp": ("strip_batch_fits(",)}
    for name, calls in uses.items():
        text = src(name)
        for c in calls:
            assert c in text, (name, c)
    prog = open(os.path.join(ROOT, "tests", "cpp", "grid_plan.cpp")).read()
    consts = dict(re.findall(r"\b(k\w+) = (\d+)", re.search(r"constexpr int kCcTileW[^;]*;", prog).group(0)))
    comp, chains, contour = src("cvs_components.h"), src("cvs_chains.h") + src("cvs_kernels_chains.hip"), src("cvs_kernels_contour.hip")
    for name, text in (("kCcTileW", comp), ("kCcTileH", comp), ("kChRows", chains), ("kHystTileW", contour), ("kHystTileH", contour)):
        m = re.search(r"\b%s = (\d+)" % name, text)
        assert m and m.group(1) == consts[name], name
    assert "kNmsSpan = 62" in contour and "grid_ceil_div(cols, 62)" in hdr
