"""tests/roi_guard.py proven before it is trusted (no GPU): a numpy surrogate "kernel" that writes rows x cols into views of guarded
parents, with one-line faults switched on in turn, driven exactly as tests/test_gpu_roi_footprint.py drives the engine; and the coverage
ledger, held to the set of entry points parsed from include/cvsteer_hip.h."""
import os

import numpy as np
import pytest

import roi_guard as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAULTS = {
    "a": "one column too many in every row",
    "b": "cols rounded up to 4 in the last row only",
    "c": "one row too many below",
    "d": "one row too many above",
    "e": "a dense copy that ignores the pitch",
    "f": "the neighbouring window's output touched (side by side)",
    "g": "the input modified",
    "h": "the input's left neighbour added into column 0",
    "i": "bytes: a whole dword stored at the row end",
}
DTYPES = (np.float32, np.uint8, np.int32)
SHAPES = ((5, 7), (4, 8))      # cols % 4 != 0 and == 0


def _flat(parent, k=0):
    """(flat memory of the parent, offset of view k's first element, pitch in elements, rows, cols)"""
    r, c = parent.windows[k]
    return parent.buf.reshape(-1), r.start * parent.shape[1] + c.start, parent.shape[1], r.stop - r.start, c.stop - c.start


def _op(x, which):
    """the surrogate's arithmetic: two outputs per call"""
    if x.dtype == np.float32:
        return x * np.float32(2) + np.float32(1) if which == 0 else x - np.float32(1)
    if x.dtype == np.uint8:
        return x ^ np.uint8(0x3C if which == 0 else 0xC3)
    return x + np.int32(7 if which == 0 else -7)


def surrogate(pin, pouts, fault=None):
    """out_k[r][c] = op_k(in[r][c]) by pointer arithmetic on the parents' flat memory, like a kernel: base + r * pitch + c"""
    src, sb, sp, rows, cols = _flat(pin)
    for k in reversed(range(len(pouts))):            # (window 0 last: what fault f writes into window 1 stays)
        parent, w = pouts[k] if isinstance(pouts[k], tuple) else (pouts[k], 0)
        dst, db, dp, _, _ = _flat(parent, w)
        for r in range(rows):
            n = cols
            if fault == "a" and k == 0:
                n = cols + 1
            if fault == "b" and k == 0 and r == rows - 1:
                n = (cols + 3) // 4 * 4
            if fault == "i" and k == 0 and dst.dtype == np.uint8:
                n = (cols + 3) // 4 * 4
            val = np.zeros(n, dst.dtype)
            val[:cols] = _op(src[sb + r * sp:sb + r * sp + cols], k)
            if fault == "h" and k == 0:
                at = max(sb + r * sp - 1, 0)
                val[:1] = val[:1] + src[at:at + 1]
            at = db + r * (cols if (fault == "e" and k == 0) else dp)
            dst[at:at + n] = val
        if k == 0 and fault == "c":
            dst[db + rows * dp:db + rows * dp + cols] = 0
        if k == 0 and fault == "d":
            dst[db - dp:db - dp + cols] = 0
        if k == 0 and fault == "f" and isinstance(pouts[1], tuple) and pouts[1][0] is parent:
            assert _flat(parent, 1)[1] == db + cols + 1
            dst[db + cols + 1] = 0                   # one element past the gutter: the neighbour's column 0
    if fault == "g":
        src[sb] = _op(src[sb:sb + 1], 0)[0]


def drive(dtype, shape, placement, fault):
    """What the GPU driver does with an entry point: the call on guarded views against the correct call on dense planes, then the four
    checks.  Returns the names of the checks that failed."""
    rng = np.random.default_rng(7)
    x = (rng.random(shape) * 200).astype(dtype)
    dense_in = G.Parent(shape, dtype)
    dense_in.claim((slice(0, shape[0]), slice(0, shape[1])))[...] = x
    dense = [G.Parent(shape, dtype) for _ in range(2)]
    for d in dense:
        d.claim((slice(0, shape[0]), slice(0, shape[1])))
    surrogate(dense_in, dense)
    want = [d.buf.copy() for d in dense]
    failed, results = [], []
    for surround in (G.BYTE_SURROUNDS if np.dtype(dtype) == np.uint8 else (None,)):
        pin, _ = G.guard_input(x, placement, surround=surround)
        parents, views = G.windows([(shape, dtype)] * 2, placement)
        pouts = [(parents[0], 0), (parents[0], 1)] if len(parents) == 1 else parents
        surrogate(pin, pouts, fault)
        results.append([v.copy() for v in views])
        for check, label in ((lambda: G.assert_same_bits(views, want), "values"),
                             (lambda: [G.assert_frame_intact(p) for p in parents], "frame"),
                             (lambda: G.assert_inputs_intact(pin), "input")):
            try:
                check()
            except AssertionError:
                failed.append(label)
    if len(results) == 2:
        try:
            G.assert_same_bits(results[0], results[1])
        except AssertionError:
            failed.append("footprint")
    return sorted(set(failed))


def can_show(fault, dtype, shape, placement):
    if fault in ("b", "i") and shape[1] % 4 == 0:
        return False
    if fault == "i" and np.dtype(dtype) != np.uint8:
        return False
    if fault == "f":
        return placement == "side"
    return True


def _placements(dtype):
    return G.PLACEMENTS + (G.BYTE_PLACEMENTS if np.dtype(dtype) == np.uint8 else ())


def test_margins_are_what_the_names_say():
    for cols in (1, 5, 67, 260):
        t, b, l, r = G.margins("aligned", cols, np.float32)
        assert (t, b) == (2, 3) and l % 4 == 0 and (l + cols + r) % 4 == 0
        t, b, l, r = G.margins("aligned", cols, np.uint8)
        assert l % 16 == 0 and (l + cols + r) % 16 == 0
        t, b, l, r = G.margins("odd", cols, np.float32)
        assert (l, r >= 5) == (3, True) and (l + cols + r) % 2 == 1 and t >= 1 and b >= 1
        assert G.margins("tight", cols, np.float32) == (1, 1, 0, 1)
        assert G.margins("wide", cols, np.int32) == (32, 32, 64, 64)
        for k in (1, 2, 3):
            assert G.margins("off%d" % k, cols, np.uint8)[2] == k
    p, v = G.window((3, 8), np.float32, "aligned")
    assert v.ctypes.data % 16 == 0 and v.strides[0] % 16 == 0
    parents, views = G.windows([((3, 5), np.float32), ((3, 4), np.float32), ((3, 5), np.uint8)], "side")
    assert len(parents) == 2 and views[1].ctypes.data - views[0].ctypes.data == 6 * 4 and views[0].strides == views[1].strides


def test_sentinels_are_compared_as_bits():
    p, v = G.window((2, 3), np.float32, "tight")
    assert np.isnan(p.buf).all() and (p.bits() == G.F32_SENTINEL_BITS).all()
    v[...] = np.nan                                  # an output may hold NaN of its own
    G.assert_frame_intact(p)
    p.buf[0, 0] = np.nan                             # another NaN in the frame: not the sentinel
    with pytest.raises(AssertionError, match=r"\(row, column\) = \(-1, 0\)"):
        G.assert_frame_intact(p)
    q, _ = G.window((2, 3), np.uint8, "off2")
    assert (q.bits() == 0xA5).all()
    q.buf[1, 2 + 3] = 0
    with pytest.raises(AssertionError, match=r"1 element\(s\).*\(0, 3\)"):
        G.assert_frame_intact(q)
    s, _ = G.window((2, 3), np.int32, "odd")
    assert (s.buf == 0x5A5A5A5A).all()
    a, av = G.array((5, 2), np.int32, 3, 4)
    assert av.shape == (5, 2) and a.shape == (12, 2)
    a.buf[8, 1] = 0
    with pytest.raises(AssertionError):
        G.assert_frame_intact(a)
    b, inner = G.block((3, 2, 4, 6), 2, "odd")
    assert inner.shape == (3, 2, 4, 6) and b.shape == (3, 2, 7, 15)
    inner[...] = 1.0
    G.assert_frame_intact(b)


def test_correct_surrogate_is_clean_and_every_fault_is_caught(capsys):
    table = {}
    for dtype in DTYPES:
        for shape in SHAPES:
            for placement in _placements(dtype):
                assert drive(dtype, shape, placement, None) == [], (dtype, shape, placement)
                for fault in FAULTS:
                    failed = drive(dtype, shape, placement, fault)
                    shows = can_show(fault, dtype, shape, placement)
                    assert bool(failed) == shows, (fault, FAULTS[fault], np.dtype(dtype).name, shape, placement, failed)
                    if shows:
                        table.setdefault((fault, placement), set()).update(failed)
    caught = {f for f, _ in table}
    assert caught == set(FAULTS), sorted(set(FAULTS) - caught)
    for fault in FAULTS:                             # every placement that can show a fault has shown it
        for dtype in DTYPES:
            for placement in _placements(dtype):
                if any(can_show(fault, dtype, s, placement) for s in SHAPES):
                    assert (fault, placement) in table, (fault, placement)
    with capsys.disabled():
        print("\nfault by placement (which check caught it; - = the placement cannot show it)")
        print("%-6s" % "fault" + "".join("%-17s" % p for p in G.ALL_PLACEMENTS))
        for fault in FAULTS:
            print("%-6s" % fault + "".join("%-17s" % ("+".join(sorted(table[(fault, p)])) if (fault, p) in table else "-") for p in G.ALL_PLACEMENTS))


def test_byte_neighbour_reads_need_both_surroundings():
    """fault h on bytes: with 0x00 around the view the sum is unchanged -- only the second run, 0xFF around it, shows the read"""
    assert drive(np.uint8, (5, 7), "odd", "h") != []
    x = np.full((5, 7), 3, np.uint8)
    pin, _ = G.guard_input(x, "odd", surround=0x00)
    parents, views = G.windows([((5, 7), np.uint8)] * 2, "odd")
    surrogate(pin, parents, "h")
    assert (views[0] == (x ^ 0x3C)).all()


def test_ledger_equals_the_header():
    with open(os.path.join(ROOT, "include", "cvsteer_hip.h")) as fh:
        declared = G.header_entry_points(fh.read())
    assert len(declared) >= 35 and "cvs_pipeline" in declared and "cvs_contour_points" in declared and "cvs_create" not in declared
    covered, exempt = set(G.COVERED), set(G.EXEMPT)
    assert len(covered) == len(G.COVERED), "a name twice in COVERED"
    assert not covered & exempt, sorted(covered & exempt)
    assert covered | exempt == declared, "undecided: %s; not in the header: %s" % (sorted(declared - covered - exempt), sorted((covered | exempt) - declared))
    assert all(isinstance(r, str) and len(r) > 10 for r in G.EXEMPT.values())
    for name in G.COVERED:                           # removing a name from COVERED fails here
        assert (set(G.COVERED) - {name}) | exempt != declared


def test_gpu_table_has_a_row_for_every_covered_name():
    """the GPU file's rows, read without a GPU: generated from COVERED, so a name without a row fails at collection -- and here"""
    import ast
    with open(os.path.join(ROOT, "tests", "test_gpu_roi_footprint.py")) as fh:
        tree = ast.parse(fh.read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and getattr(node.func, "id", "") == "row" and node.args and isinstance(node.args[0], ast.Constant):
            names.add(node.args[0].value)
    assert names == set(G.COVERED), (sorted(set(G.COVERED) - names), sorted(names - set(G.COVERED)))
