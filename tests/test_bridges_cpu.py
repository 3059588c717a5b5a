"""Contour bridges (cvs_chain_bridges) at every layer that exists without a GPU: the public header, the exports and the Python surface,
the generated code of the new kernels (no scratch memory), and the model of bridges_model.py that the GPU tests hold the kernels against --
dashed lines with known answers, pairs that must not bridge, the composition with the join and path models, and the shape of the random
and crowded inputs the GPU tests use."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bridges_cases as BC
import bridges_model as M
import joins_model as JM
import paths_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "cvsteer_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
F32 = np.float32
OFFSETS = dict(partner=0, flags=4, n=8, steps=12, bridge=16, start=20, cos=24, cos_partner=28)
CFG_OFFSETS = dict(radius=0, min_arm=4, max_gap=8, min_cos=12)


# ---- header, binding and build ----
def test_header_declares_the_call_and_the_records(tmp_path):
    text = open(os.path.join(ROOT, "include", "cvsteer_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int cvs_chain_bridges\(([^;]*)\);", plain)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == (
        "cvs_handle h, const int32_t* points, int n_points, const cvs_chain* chains, int n_chains, const float* xy, "
        "const cvs_bridge_cfg* cfg, cvs_chain_bridge* table, int32_t* out_points, int cap_points, cvs_chain* out_chains, int cap_chains, "
        "float* out_xy, int32_t* counts, int mem")
    src = os.path.join(str(tmp_path), "use.cpp")
    with open(src, "w") as f:
        f.write('#include <stddef.h>\n#include "cvsteer_hip.h"\n'
                'static_assert(sizeof(cvs_chain_bridge) == 32 && sizeof(cvs_bridge_cfg) == 16, "sizes");\n'
                'static_assert(CVS_BRIDGE_MUTUAL == 1 && CVS_BRIDGE_NONE == 2 && CVS_BRIDGE_JUNCTION == 4 && CVS_BRIDGE_SHORT == 8 && '
                'CVS_BRIDGE_DEGENERATE == 16 && CVS_BRIDGE_NO_CHAIN == 32 && CVS_BRIDGE_CROWDED == 64, "flags");\n'
                + "".join('static_assert(offsetof(cvs_bridge_cfg, %s) == %d, "%s");\n' % (n, o, n) for n, o in CFG_OFFSETS.items())
                + "".join('static_assert(offsetof(cvs_chain_bridge, %s) == %d, "%s");\n' % (n, o, n) for n, o in OFFSETS.items()) +
                'int main() { return cvs_chain_bridges == 0; }\n')
    subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), src], check=True)
    # the scratch the header names is the one the kernels' header computes, and the build lists name the units
    hdr = open(os.path.join(SRC, "cvs_bridges.h")).read()
    assert "kBridgeEndBytes = 120" in hdr and "kBridgeChainBytes = 2 * kBridgeEndBytes + 4" in hdr and "CVS_BRIDGE_SCRATCH_PER_CHAIN = 244" in plain
    make = open(os.path.join(SRC, "Makefile")).read()
    units = dict(re.findall(r"^(HOST_UNITS|KERNEL_UNITS)\s*=\s*(.*)$", make, re.M))
    assert "cvs_bridges" in units["HOST_UNITS"].split() and "cvs_kernels_bridges" in units["KERNEL_UNITS"].split()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "bridging gaps between free ends" not in readme and "cvs_chain_bridges" in readme


def test_libraries_export_and_bind():
    import cvsteer_amd
    from cvsteer_amd import _lib as L
    res, args = L.SIGNATURES["cvs_chain_bridges"]
    assert res is C.c_int and len(args) == 15 and args[6] == C.POINTER(L.BridgeCfg) and args[-1] is C.c_int
    assert C.sizeof(L.ChainBridge) == 32 == M.BRIDGE_DTYPE.itemsize and C.sizeof(L.BridgeCfg) == 16
    names = ("MUTUAL", "NONE", "JUNCTION", "SHORT", "DEGENERATE", "NO_CHAIN", "CROWDED")
    assert [getattr(L, "BRIDGE_" + n) for n in names] == [getattr(M, n) for n in names] == [getattr(cvsteer_amd, "BRIDGE_" + n) for n in names]
    assert (L.BRIDGE_SCRATCH_PER_CHAIN, L.BRIDGE_MAX_GAP, L.BRIDGE_MAX_CELL) == (244, 32, M.MAX_CELL)
    hip = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "cvsteer_amd", "libcvsteer_hip.so")], text=True)
    assert re.search(r" T cvs_chain_bridges$", hip, re.M)
    assert cvsteer_amd.BRIDGE_DTYPE == M.BRIDGE_DTYPE
    for cls in (cvsteer_amd.SteerableFiltersG2, cvsteer_amd.SteerableFiltersG4):
        assert all(callable(getattr(cls, name, None)) for name in ("chain_bridges", "contour_bridges"))
        assert cls.BRIDGE_DTYPE == M.BRIDGE_DTYPE and {n: cls.BRIDGE_DTYPE.fields[n][1] for n in cls.BRIDGE_DTYPE.names} == OFFSETS
    assert [(n, getattr(L.ChainBridge, n).offset) for n, _ in L.ChainBridge._fields_] == list(OFFSETS.items())
    assert [(n, getattr(L.BridgeCfg, n).offset) for n, _ in L.BridgeCfg._fields_] == list(CFG_OFFSETS.items())


def test_null_handle():
    from cvsteer_amd import _lib as L
    pts, tab = np.int32([[0, 0], [1, 0], [2, 0]]), np.int32([[0, 3, 0, 0]])
    rec, counts = np.full((2, 8), -9, np.int32), np.full(3, -9, np.int32)
    cfg = L.BridgeCfg(1, 1, 2, -1.0)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert L.lib().cvs_chain_bridges(None, p(pts), 3, p(tab), 1, None, C.byref(cfg), p(rec), None, 0, None, 0, None, p(counts), L.MEM_HOST) == L.E_BADARG
    assert (rec == -9).all() and (counts == -9).all()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_bridge_kernels_use_no_scratch(tmp_path):
    path = os.path.join(str(tmp_path), "cvs_kernels_bridges.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    "-I" + SRC, "-S", "--cuda-device-only", os.path.join(SRC, "cvs_kernels_bridges.hip"), "-o", path], check=True,
                   stderr=subprocess.DEVNULL)
    text = open(path).read()
    scratch = {}
    for blk in text.split("  - .agpr_count:")[1:]:
        nm = re.search(r"\.name:\s+(\S+)", blk)
        ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        if nm and ps:
            scratch[nm.group(1)] = int(ps.group(1))
    stems = ("k_bridge_arms", "k_bridge_insert", "k_bridge_crowd", "k_bridge_best", "k_bridge_resolve", "k_bridge_records", "k_bridge_emit")
    for stem in stems:
        assert any(stem in n for n in scratch), (stem, sorted(scratch))
    assert len(scratch) == len(stems) and all(v == 0 for v in scratch.values()), scratch


# ---- the model: dashed lines ----
def _ends_pixel(pts, chains, e):
    return tuple(pts[chains[e >> 1, 0] + (chains[e >> 1, 1] - 1) * (e & 1)].tolist())


@pytest.mark.parametrize("kind", ["horizontal", "vertical", "diagonal"])
def test_dashed_line_one_bridge_per_gap(kind):
    pts, chains, xy = BC.cases()[kind]
    dashes = BC.dashed_pixels(kind)[2]
    assert chains[:, 1].tolist() == [BC.DASH] * dashes and (chains[:, 2] == 0).all()
    table, o_pts, o_chn, o_xy, counts = M.bridges(pts, chains, radius=8, min_arm=3, max_gap=4, min_cos=0.8)
    gaps = dashes - 1
    assert counts == (gaps, dashes + gaps, len(pts) + gaps * (BC.GAP + 2)) and o_xy is None
    assert len(o_pts) == counts[2] and len(o_chn) == counts[1]
    assert np.array_equal(o_pts[:len(pts)], pts) and np.array_equal(o_chn[:dashes, [0, 1, 3]], chains[:, [0, 1, 3]])
    mutual = np.nonzero(table["flags"] & M.MUTUAL)[0]
    assert len(mutual) == 2 * gaps and (table["flags"][mutual] == M.MUTUAL).all() and (table["steps"][mutual] == BC.GAP + 1).all()
    assert (table["cos"][mutual] == 1.0).all() and (table["cos_partner"][mutual] == 1.0).all() and (table["n"] == BC.DASH - 1).all()
    free = np.setdiff1d(np.arange(2 * dashes), mutual)
    assert len(free) == 2 and (table["flags"][free] == 0).all() and (table["partner"][free] == -1).all()   # the two outer ends
    assert (table["bridge"][free] == -1).all() and (table["start"][free] == -1).all() and (table["steps"][free] == 0).all()
    assert (table["cos"].view(np.uint32)[free] == M.QNAN_BITS).all()
    flags = o_chn[:dashes, 2].tolist()                                          # every bridged end now reads as a junction
    assert sorted(flags) == sorted([M.HEAD_JUNCTION, M.TAIL_JUNCTION] + [M.HEAD_JUNCTION | M.TAIL_JUNCTION] * (dashes - 2))
    for k in range(gaps):
        lo = int(np.nonzero((table["bridge"] == k) & (np.arange(len(table)) < table["partner"]))[0][0])
        hi = int(table["partner"][lo])
        s, ln, fl, r = o_chn[dashes + k].tolist()
        assert (s, ln, fl, r) == (int(table["start"][lo]), BC.GAP + 2, M.HEAD_JUNCTION | M.TAIL_JUNCTION, 0) and table["start"][hi] == s
        line = o_pts[s:s + ln]
        assert tuple(line[0].tolist()) == _ends_pixel(pts, chains, lo) and tuple(line[-1].tolist()) == _ends_pixel(pts, chains, hi)
        assert (np.abs(np.diff(line, axis=0)).max(axis=1) == 1).all()           # 8-connected
    assert sorted(map(tuple, o_pts.tolist())) == sorted(BC.dashed_pixels(kind)[1] + [_ends_pixel(pts, chains, e) for e in mutual])
    # no bridge at max_gap 2, and the sub-pixel positions of a bridge lie between those of its ends
    none = M.bridges(pts, chains, radius=8, min_arm=3, max_gap=2, min_cos=0.8)
    assert none[4] == (0, dashes, len(pts)) and not (none[0]["flags"] & M.MUTUAL).any() and np.array_equal(none[2], chains)
    sub = M.bridges(pts, chains, xy, radius=8, min_arm=3, max_gap=4, min_cos=0.8)
    assert sub[4] == counts and sub[3].dtype == F32 and sub[3][:len(pts)].tobytes() == xy.tobytes()
    assert np.abs(sub[3] - sub[1]).max() <= 0.4 + 1e-6


def test_parallel_dashes_are_not_bridged():
    pts = np.int32([(x, 10) for x in range(5, 11)] + [(x, 13) for x in range(5, 11)])
    tab = np.int32([[0, 6, 0, 0], [6, 6, 0, 0]])
    table = M.bridges(pts, tab, radius=8, min_arm=3, max_gap=8, min_cos=0.8)[0]
    assert (table["flags"] == 0).all() and (table["partner"] == -1).all()
    loose = M.bridges(pts, tab, radius=8, min_arm=3, max_gap=8, min_cos=-1.0)[0]  # the cone is what keeps them apart
    assert (loose["flags"] == M.MUTUAL).all() and loose["partner"].tolist() == [2, 3, 0, 1] and (loose["cos"] == 0.0).all()


def test_of_three_collinear_candidates_the_nearer_pair_wins():
    """A's tail at x = 7 looks right; the heads of B (x = 10) and C (x = 12) both look left at it: A and B pair off, C is left over with a
    partner that does not agree"""
    row = lambda x0: [(x, 10) for x in range(x0, x0 + 6)]
    pts, tab = np.int32(row(2) + row(10) + row(12)), np.int32([[0, 6, 0, 0], [6, 6, 0, 0], [12, 6, 0, 0]])
    table, o_pts, o_chn, _, counts = M.bridges(pts, tab, radius=8, min_arm=3, max_gap=8, min_cos=0.8)
    assert table["partner"].tolist() == [-1, 2, 1, -1, 1, -1] and table["flags"].tolist() == [0, M.MUTUAL, M.MUTUAL, 0, 0, 0]
    assert table["steps"].tolist() == [0, 3, 3, 0, 5, 0] and table["bridge"].tolist() == [-1, 0, 0, -1, -1, -1] and counts == (1, 4, 22)
    assert o_pts[18:].tolist() == [[7, 10], [8, 10], [9, 10], [10, 10]] and o_chn[3].tolist() == [18, 4, 6, 0]


def test_a_c_closes_on_itself():
    """one open chain round a rectangle, its two ends facing each other across a gap of three pixels on the top side"""
    ring = ([(x, 5) for x in range(12, 16)] + [(15, y) for y in range(6, 13)] + [(x, 12) for x in range(14, 4, -1)]
            + [(5, y) for y in range(11, 4, -1)] + [(x, 5) for x in range(6, 9)])
    pts, tab = np.int32(ring), np.int32([[0, len(ring), 0, 0]])
    table, o_pts, o_chn, _, counts = M.bridges(pts, tab, radius=3, min_arm=3, max_gap=4, min_cos=0.8)
    assert table["partner"].tolist() == [1, 0] and (table["flags"] == M.MUTUAL).all() and (table["steps"] == 4).all() and counts == (1, 2, len(ring) + 5)
    assert o_pts[len(ring):].tolist() == [[12, 5], [11, 5], [10, 5], [9, 5], [8, 5]]
    assert o_chn.tolist() == [[0, len(ring), 6, 0], [len(ring), 5, 6, 0]]
    joins = JM.joins(o_pts, o_chn, radius=3, min_arm=3)
    r = PM.paths(o_pts, o_chn, joins)
    assert r["cycles"] == [True] and r["paths"].tolist() == [[0, len(ring) + 3, PM.CLOSED, 0]]
    assert len({tuple(p) for p in r["path_points"].tolist()}) == len(ring) + 3   # every pixel of the closed contour once


@pytest.mark.parametrize("kind", ["horizontal", "vertical", "diagonal"])
def test_joins_and_paths_stitch_through_the_bridges(kind):
    pts, chains, _ = BC.cases()[kind]
    _, o_pts, o_chn, _, _ = M.bridges(pts, chains, radius=8, min_arm=3, max_gap=4, min_cos=0.8)
    joins = JM.joins(o_pts, o_chn, radius=8, min_arm=3)
    live = joins["degree"][joins["node"] >= 0]
    assert sorted(np.bincount(live).tolist()) == sorted([0, 2, len(live) - 2])    # the two outer ends, every other end at a node of two
    r = PM.paths(o_pts, o_chn, joins)
    whole = BC.dashed_pixels(kind)[1]
    assert r["counts"] == (1, len(whole)) and r["paths"].tolist() == [[0, len(whole), 0, 0]]
    assert list(map(tuple, r["path_points"].tolist())) == whole                 # the line, in order, each pixel once


# ---- the inputs of the GPU tests ----
def test_gpu_inputs_have_every_kind_of_end():
    cases = BC.cases()
    for name in ("random 0.05", "random 0.20"):
        pts, chains, xy = cases[name]
        seen = 0
        for radius, min_arm, max_gap, min_cos in BC.CONFIGS:
            for sub in (None, xy):
                table, o_pts, o_chn, o_xy, counts = M.bridges(pts, chains, sub, radius=radius, min_arm=min_arm, max_gap=max_gap, min_cos=min_cos)
                seen |= int(np.bitwise_or.reduce(table["flags"]))
                mutual = np.nonzero(table["flags"] & M.MUTUAL)[0]
                assert (table["partner"][table["partner"][mutual]] == mutual).all() and len(mutual) == 2 * counts[0]
                assert (table["cos"].view(np.uint32)[mutual] == table["cos_partner"].view(np.uint32)[table["partner"][mutual]]).all()
                assert counts[1] == len(chains) + counts[0] == len(o_chn) and counts[2] == len(o_pts)
                assert not JM.host_table_wrong(len(o_pts), o_chn)               # again a table every chain call takes
        assert seen & M.MUTUAL and seen & M.JUNCTION and seen & M.SHORT and not seen & M.NO_CHAIN, (name, seen)
        assert bool(seen & M.CROWDED) == (name == "random 0.20")                   # (at max_gap 32 the denser mask fills a cell past 32)
    pts, chains, xy = cases["crowd"]
    table = M.bridges(pts, chains, radius=1, min_arm=1, max_gap=8, min_cos=0.8)[0]
    assert (table["flags"][:92] == M.CROWDED).all() and (table["partner"][:92] == -1).all()   # the cell of 80 and its neighbour
    assert table["flags"][92:].tolist() == [0, M.MUTUAL, M.MUTUAL, 0] * 2 and table["partner"][92:].tolist() == [-1, 94, 93, -1, -1, 98, 97, -1]
    assert M.bridges(pts, chains, radius=1, min_arm=1, max_gap=2, min_cos=0.8)[0]["flags"].max() < M.CROWDED   # smaller cells: nobody is crowded
    # two planes never meet; negative coordinates change nothing but the coordinates
    pts2, chains2, xy2 = BC.two_planes()
    t2 = M.bridges(pts2, chains2, radius=8, min_arm=3, max_gap=4, min_cos=0.8)[0]
    one = M.bridges(*cases["horizontal"][:2], radius=8, min_arm=3, max_gap=4, min_cos=0.8)[0]
    m = len(one)
    assert np.array_equal(t2["partner"][:m], one["partner"]) and np.array_equal(t2["partner"][m:], np.where(one["partner"] >= 0, one["partner"] + m, -1))
    flat = np.array(chains2)
    flat[:, 3] = 0
    assert not np.array_equal(M.bridges(pts2, flat, radius=8, min_arm=3, max_gap=4, min_cos=0.8)[0]["partner"], t2["partner"])
    for name in ("diagonal", "random 0.20"):
        base = M.bridges(*cases[name][:2], radius=8, min_arm=3, max_gap=5, min_cos=0.8)
        moved = M.bridges(*BC.shifted(name, -37, -29)[:2], radius=8, min_arm=3, max_gap=5, min_cos=0.8)
        assert base[4] == moved[4] and (base[0]["flags"] & M.MUTUAL).any()
        assert np.array_equal(moved[1], base[1] + np.int32([-37, -29])) and np.array_equal(moved[2], base[2])
        assert np.array_equal(moved[0]["partner"], base[0]["partner"])
