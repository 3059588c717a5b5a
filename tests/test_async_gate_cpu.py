"""The pure logic of tests/async_gate.py (no GPU): calibration arithmetic, the 250 ms refusal, the poison and sentinel makers."""
import numpy as np
import pytest

import async_gate as G


def test_calibration_arithmetic():
    assert G.cycles_per_ms(20_000_000, 10.0) == 2_000_000.0
    assert G.units_for(50.0, 2_000_000.0) == 100_000_000
    assert G.units_for(0.0001, 1.0) == 1   # never an empty delay
    for bad in ((0, 1.0), (100, 0.0), (100, -1.0), (100, float("nan"))):
        with pytest.raises(ValueError):
            G.cycles_per_ms(*bad)


def test_delays_above_the_cap_are_refused():
    assert G.MAX_MS == 250.0 and G.START_MS == 50.0
    G.units_for(250.0, 10.0)
    for ms in (250.001, 1000.0, 0.0, -5.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            G.units_for(ms, 10.0)
    with pytest.raises(ValueError):   # a Section refuses before anything is queued (no stream is touched)
        G.Section(None, ms=251.0)
    with pytest.raises(ValueError):
        G.behind(None, ms=300.0)


def test_poison_and_sentinel():
    f = G.poison_like(np.zeros((3, 5), np.float32))
    assert f.dtype == np.float32 and f.shape == (3, 5) and np.isnan(f).all()
    d = G.poison_like(np.zeros(4, np.float64))
    assert d.dtype == np.float64 and np.isnan(d).all()
    b = G.poison_like(np.zeros((2, 7), np.uint8))
    assert b.dtype == np.uint8 and (b == 0xA5).all()
    i = G.poison_like(np.zeros((6, 2), np.int32))
    assert i.dtype == np.int32 and i.shape == (6, 2) and (i.view(np.uint8) == 0xA5).all() and (i < 0).all()   # no valid coordinate
    b[0, 0] = 1   # writable copies
    s = G.sentinel((2, 3), np.float32)
    assert s.dtype == np.float32 and (s == G.SENTINEL_F32).all()
    u = G.sentinel((5,), np.uint8)
    assert (u == G.SENTINEL_BYTE).all()
    t = G.sentinel((3, 40), np.uint8)
    assert t.shape == (3, 40) and (t == 0x5A).all()
    k = G.sentinel((4,), np.int32)
    assert (k.view(np.uint8) == 0x5A).all()
    assert G.sentinel((0, 2), np.int32).shape == (0, 2) and G.poison_like(np.zeros((0, 2), np.float32)).shape == (0, 2)
