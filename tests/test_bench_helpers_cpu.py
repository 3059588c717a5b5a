"""CPU tests of bench.py's host-side helpers (no GPU): the median, the telemetry lookup, the guard of the live counter passes."""
import importlib.util
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_median(bench):
    assert bench._median([3.0, 1.0, 2.0]) == 2.0
    assert bench._median([4.0, 1.0, 3.0, 2.0]) == 2.5
    assert bench._median([7.0]) == 7.0


def test_telemetry_lookup_without_a_device_is_none(bench):
    """no HIP device (or a card whose hwmon files cannot be matched by PCI address): no telemetry block, no exception"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("needs a machine without a GPU")
    assert bench._telemetry_files(torch, 0) is None


def test_live_counter_passes_refuse_to_nest_under_a_profiler(bench, monkeypatch):
    """bench.py under rocprofv3 (tools/profile.sh) must not start rocprofv3 children of its own"""
    monkeypatch.setenv("ROCPROFILER_TEST_MARK", "1")
    got, why = bench._live_traffic()
    assert got is None and "profiler" in why
    monkeypatch.delenv("ROCPROFILER_TEST_MARK")
    monkeypatch.setenv("LD_PRELOAD", "/opt/rocm/lib/librocprofiler-sdk-tool.so")
    got, why = bench._live_traffic()
    assert got is None and "profiler" in why


def test_full_is_an_option():
    """everything beyond the headline sits behind --full, which --help names (argparse answers before torch is imported)"""
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--full" in r.stdout, r.stdout


def test_bytes_per_pixel_table_matches_the_survey(bench):
    """SURVEY.md 8(d) / DESIGN.md 3: algorithmic bytes per pixel of the timed legs"""
    b = bench.BYTES_PER_PIX
    assert (b["M1"], b["M2"], b["M4"], b["M5"], b["M6"], b["M6s"]) == (32, 40, 52, 84, 48, 56)
    assert b["M2_u8"] == 37 and b["C4_u8_feat3"] == 13


def test_dump_rows_are_fixed_distinct_and_hold_the_edges(bench):
    """--dump-outputs writes the same rows in every run: both 8-row edges and a seeded sample of the rest, within the 64 MB cap"""
    import numpy as np
    r = bench._dump_rows()
    assert np.array_equal(r, bench._dump_rows())
    assert len(r) == bench.DUMP_ROWS and np.all(np.diff(r) > 0) and 0 <= r[0] and r[-1] < bench.ROWS
    assert set(range(8)) | set(range(bench.ROWS - 8, bench.ROWS)) <= set(r.tolist())
    assert 2 * len(r) * bench.COLS * 4 <= 64e6     # g and h, float32


def test_dump_outputs_writes_the_named_rows_as_float32(bench, tmp_path):
    import numpy as np
    import torch
    plane = torch.arange(bench.ROWS, dtype=torch.float32)[:, None].expand(bench.ROWS, bench.COLS)   # every pixel holds its row index
    bench._dump_outputs(torch, str(tmp_path / "d"), {"g": plane, "h": -plane})
    g, h = np.load(tmp_path / "d" / "g.npy"), np.load(tmp_path / "d" / "h.npy")
    assert g.dtype == h.dtype == np.float32 and g.shape == h.shape == (bench.DUMP_ROWS, bench.COLS)
    assert np.array_equal(g[:, 0], bench._dump_rows().astype(np.float32)) and np.array_equal(h, -g)
    assert (g == g[:, :1]).all()
