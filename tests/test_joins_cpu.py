"""Contour joins (cvs_chain_joins) at every layer that exists without a GPU: the public header, the exports of both libraries, the Python
surface, the generated code of the new kernels (no scratch), the host table check under the host sanitizers as a stand-alone program, and
the model of joins_model.py that the GPU tests hold the kernels against -- hand-made junctions with known answers, the structure of the
nodes of random masks, and the ridge that turns by 120 degrees, whose corner the joins recover."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import chains_model as CM
import joins_model as M
import turns_model as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "cvsteer_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
F32 = np.float32
OFFSETS = dict(node=0, degree=4, next=8, partner=12, flags=16, n=20, cos=24, sin=28)
CFG_OFFSETS = dict(radius=0, min_arm=4, min_cos=8, reserved=12)


# ---- header, binding and build ----
def test_header_declares_the_call_and_the_records(tmp_path):
    text = open(os.path.join(ROOT, "include", "cvsteer_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int cvs_chain_joins\(([^;]*)\);", plain)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == (
        "cvs_handle h, const int32_t* points, int n_points, const cvs_chain* chains, int n_chains, const float* xy, "
        "const cvs_join_cfg* cfg, cvs_chain_join* table, int mem")
    assert "cvs_plane" not in m.group(1) and "capacity" not in m.group(1)       # arrays and counts only: the ROI ledger is untouched
    assert re.search(r"#define CVS_ABI_VERSION 2\b", text)
    src = os.path.join(str(tmp_path), "use.cpp")
    with open(src, "w") as f:
        f.write('#include <stddef.h>\n#include "cvsteer_hip.h"\n'
                'static_assert(sizeof(cvs_chain_join) == 32 && sizeof(cvs_join_cfg) == 16, "sizes");\n'
                'static_assert(CVS_JOIN_MUTUAL == 1 && CVS_JOIN_NONE == 2 && CVS_JOIN_CROWDED == 4 && CVS_JOIN_SHORT == 8 && '
                'CVS_JOIN_DEGENERATE == 16 && CVS_JOIN_NO_CHAIN == 32, "flags");\n'
                + "".join('static_assert(offsetof(cvs_join_cfg, %s) == %d, "%s");\n' % (n, o, n) for n, o in CFG_OFFSETS.items())
                + "".join('static_assert(offsetof(cvs_chain_join, %s) == %d, "%s");\n' % (n, o, n) for n, o in OFFSETS.items()) +
                'int (*joins)(cvs_handle, const int32_t*, int, const cvs_chain*, int, const float*, const cvs_join_cfg*, cvs_chain_join*, int)'
                ' = cvs_chain_joins;\n'
                'int main() { return joins == 0; }\n')
    subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), src], check=True)


def test_libraries_export_and_bind():
    import cvsteer_amd
    from cvsteer_amd import _lib as L
    assert L.SIGNATURES["cvs_chain_joins"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(L.JoinCfg),
                                                         C.c_void_p, C.c_int])
    assert C.sizeof(L.ChainJoin) == 32 == M.JOIN_DTYPE.itemsize and C.sizeof(L.JoinCfg) == 16
    assert (L.JOIN_MUTUAL, L.JOIN_NONE, L.JOIN_CROWDED, L.JOIN_SHORT, L.JOIN_DEGENERATE, L.JOIN_NO_CHAIN) \
        == (M.MUTUAL, M.NONE, M.CROWDED, M.SHORT, M.DEGENERATE, M.NO_CHAIN) \
        == (cvsteer_amd.JOIN_MUTUAL, cvsteer_amd.JOIN_NONE, cvsteer_amd.JOIN_CROWDED, cvsteer_amd.JOIN_SHORT, cvsteer_amd.JOIN_DEGENERATE,
            cvsteer_amd.JOIN_NO_CHAIN)
    hip = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "cvsteer_amd", "libcvsteer_hip.so")], text=True)
    assert re.search(r" T cvs_chain_joins$", hip, re.M)
    so = os.path.join(ROOT, "cvsteer_amd", "libcvsteer.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cvsteer_amd", "facade"), "-s"])
    syms = subprocess.check_output(["nm", "-DC", "--defined-only", so], text=True)
    for cls in ("SteerableFiltersG2", "SteerableFiltersG4"):
        assert re.search(r" T fa::%s::joinContours\(fa::Mat1f const&, std::vector<std::vector<fa::Point," % cls, syms), cls
    for cls in (cvsteer_amd.SteerableFiltersG2, cvsteer_amd.SteerableFiltersG4):
        assert all(callable(getattr(cls, name, None)) for name in ("chain_joins", "contour_joins"))
        assert cls.JOIN_DTYPE == M.JOIN_DTYPE
        assert {n: cls.JOIN_DTYPE.fields[n][1] for n in cls.JOIN_DTYPE.names} == OFFSETS
    assert [(n, getattr(L.ChainJoin, n).offset) for n, _ in L.ChainJoin._fields_] == list(OFFSETS.items())
    assert [(n, getattr(L.JoinCfg, n).offset) for n, _ in L.JoinCfg._fields_] == list(CFG_OFFSETS.items())


def test_null_handle():
    from cvsteer_amd import _lib as L
    pts, tab = np.int32([[0, 0], [1, 0], [2, 0]]), np.int32([[0, 3, 0, 0]])
    rec = np.full((2, 8), -9, np.int32)
    cfg = L.JoinCfg(1, 1, -1.0, 0)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert L.lib().cvs_chain_joins(None, p(pts), 3, p(tab), 1, None, C.byref(cfg), p(rec), L.MEM_HOST) == L.E_BADARG
    assert (rec == -9).all()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_join_kernels_use_no_scratch(tmp_path):
    path = os.path.join(str(tmp_path), "cvs_kernels_joins.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    "-I" + SRC, "-S", "--cuda-device-only", os.path.join(SRC, "cvs_kernels_joins.hip"), "-o", path], check=True,
                   stderr=subprocess.DEVNULL)
    text = open(path).read()
    scratch = {}
    for blk in text.split("  - .agpr_count:")[1:]:
        nm = re.search(r"\.name:\s+(\S+)", blk)
        ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        if nm and ps:
            scratch[nm.group(1)] = int(ps.group(1))
    for stem in ("k_join_arms", "k_join_insert", "k_join_resolve"):
        assert any(stem in n for n in scratch), (stem, sorted(scratch))
    assert len(scratch) == 3 and all(v == 0 for v in scratch.values()), scratch


def test_chain_table_rules_under_the_host_sanitizers(tmp_path):
    """The rules of a HOST chain table and the size of the join scratch (cvs_chain_table.h: what cvs_chain_turns and cvs_chain_joins, and
    cvs_chain_polylines, cvs_chain_measures and cvs_polyline_segments, refuse a table for), compiled without HIP into one stand-alone
    program with -fsanitize=address,undefined and run over valid and broken tables of exactly their size on the heap: a read past a table
    would end the program"""
    exe = os.path.join(str(tmp_path), "chain_table_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + SRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "chain_table_san.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "chain table OK" in r.stdout, r.stdout + r.stderr
    # the rule of both models is the same rule
    ok = np.int32([[0, 3, 0, 0], [3, 1, 1, 0], [4, 5, 0, 7]])
    for model in (M, TM):
        assert not model.host_table_wrong(9, ok) and model.host_table_wrong(10, ok) and model.host_table_wrong(8, ok)
        assert not model.host_table_wrong(0, ok[:0])
        for row, col, val in ((1, 0, 2), (1, 1, 0), (2, 1, 6), (0, 0, 1), (0, 1, -1)):
            bad = ok.copy()
            bad[row, col] = val
            assert model.host_table_wrong(9, bad), (model.__name__, row, col, val)


# ---- the model on its own: hand-made junctions ----
def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _plus():
    mask = np.zeros((9, 9), F32)
    mask[4, :], mask[:, 4] = 1, 1
    return mask


def _tee():
    mask = np.zeros((9, 9), F32)
    mask[2, :], mask[2:, 4] = 1, 1
    return mask


def _cross():
    mask = np.zeros((9, 9), F32)
    for k in range(9):
        mask[k, k], mask[k, 8 - k] = 1, 1
    return mask


@pytest.mark.parametrize("min_arm", [1, 3])
def test_model_plus(min_arm):
    pts, chains = CM.chains(_plus())
    assert chains[:, :2].tolist() == [[0, 5], [5, 5], [10, 5], [15, 5]]
    t = M.joins(pts, chains, radius=8, min_arm=min_arm)
    at = [1, 3, 4, 6]
    assert (t["node"][at] == 1).all() and (t["degree"][at] == 4).all() and t["next"][at].tolist() == [3, 4, 6, 1]
    assert t["partner"][at].tolist() == [6, 4, 3, 1] and (t["flags"][at] == M.MUTUAL).all()
    assert (t["cos"][at] == 1.0).all() and (t["sin"][at] == 0.0).all() and (t["n"] == 4).all()
    assert _bits(t["sin"][1]) ^ _bits(t["sin"][6]) == 0x80000000 and _bits(t["sin"][3]) ^ _bits(t["sin"][4]) == 0x80000000
    free = [0, 2, 5, 7]
    assert (t["degree"][free] == 1).all() and t["next"][free].tolist() == free and t["node"][free].tolist() == free
    assert (t["partner"][free] == -1).all() and (t["flags"][free] == 0).all() and (_bits(t["cos"][free]) == M.QNAN_BITS).all()
    assert (_bits(t["sin"][free]) == M.QNAN_BITS).all()


@pytest.mark.parametrize("min_arm", [1, 3])
def test_model_tee(min_arm):
    pts, chains = CM.chains(_tee())
    assert chains[:, :2].tolist() == [[0, 5], [5, 5], [10, 7]]
    t = M.joins(pts, chains, radius=8, min_arm=min_arm)
    assert pts[[4, 5, 10]].tolist() == [[4, 2]] * 3                              # ends 1, 2 and 4 at the junction
    assert t["node"][[1, 2, 4]].tolist() == [1, 1, 1] and t["next"][[1, 2, 4]].tolist() == [2, 4, 1] and (t["degree"][[1, 2, 4]] == 3).all()
    assert t["partner"][[1, 2]].tolist() == [2, 1] and (t["flags"][[1, 2]] == M.MUTUAL).all() and (t["cos"][[1, 2]] == 1.0).all()
    assert t["partner"][4] == 1 and t["cos"][4] == 0.0 and abs(t["sin"][4]) == 1.0 and t["flags"][4] == 0   # the tie goes to the smaller end
    assert _bits(t["cos"][4]) & 0x7FFFFFFF == 0
    assert M.joins(pts, chains, radius=8, min_arm=min_arm, min_cos=1.0)["flags"][[1, 2]].tolist() == [M.MUTUAL] * 2
    assert M.joins(pts, chains, radius=8, min_arm=5)["flags"][[0, 1, 2, 3]].tolist() == [M.SHORT] * 4     # the bar's arms have 4 points
    lone = M.joins(pts, chains, radius=8, min_arm=5)
    assert lone["partner"][4] == -1 and lone["flags"][4] == 0 and _bits(lone["cos"][4]) == M.QNAN_BITS     # eligible, no candidate


@pytest.mark.parametrize("min_arm", [1, 3])
def test_model_diagonal_cross(min_arm):
    pts, chains = CM.chains(_cross())
    assert chains[:, 1].tolist() == [5, 5, 5, 5]
    t = M.joins(pts, chains, radius=8, min_arm=min_arm)
    at = np.nonzero(t["degree"] == 4)[0]
    assert len(at) == 4 and (t["node"][at] == at[0]).all() and t["next"][at].tolist() == at[1:].tolist() + [int(at[0])]
    assert (t["flags"][at] == M.MUTUAL).all() and (t["cos"][at] == 1.0).all() and (t["sin"][at] == 0.0).all()
    for e in at:
        p = t["partner"][e]
        assert t["partner"][p] == e and _bits(t["sin"][e]) ^ _bits(t["sin"][p]) == 0x80000000, e
        assert (pts[chains[e // 2, 0] + (0 if e % 2 else 4)] - [4, 4]).tolist() == (-(pts[chains[p // 2, 0] + (0 if p % 2 else 4)] - [4, 4])).tolist()
    free = np.nonzero(t["degree"] == 1)[0]
    assert len(free) == 4 and t["next"][free].tolist() == free.tolist() and (t["partner"][free] == -1).all()


def test_model_records_of_chains_without_ends_and_of_broken_entries():
    pts = np.int32([[0, 0], [1, 0], [1, 1], [0, 1], [5, 5], [7, 7], [8, 7]])
    tab = np.int32([[0, 4, M.CLOSED, 0], [4, 1, 0, 0], [5, 2, 0, 0], [6, 2, 0, 0], [-1, 2, 0, 0], [3, 0, 0, 0]])
    t = M.joins(pts, tab, radius=2, min_arm=1)
    none = np.zeros(1, M.JOIN_DTYPE)
    none["node"] = none["next"] = none["partner"] = -1
    none["cos"] = none["sin"] = np.uint32(M.QNAN_BITS).view(F32)
    none["flags"] = M.NONE
    assert all(r.tobytes() == none.tobytes() for r in t[:4])                     # closed, and a single point
    none["flags"] = M.NONE | M.NO_CHAIN
    assert all(r.tobytes() == none.tobytes() for r in t[6:])                     # leaves the array, negative start, no point
    assert t["degree"][[4, 5]].tolist() == [1, 1] and t["n"][[4, 5]].tolist() == [1, 1] and t["flags"][[4, 5]].tolist() == [0, 0]


def test_model_crowded_and_planes():
    """nine two-point chains from one pixel: CROWDED; eight: resolved; the same pixel in another plane is another node"""
    spokes = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1), (2, 1)]
    for count in (8, 9):
        pts = np.int32([p for dx, dy in spokes[:count] for p in ((10, 10), (10 + dx, 10 + dy))])
        tab = np.int32([[2 * c, 2, 0, 0] for c in range(count)])
        t = M.joins(pts, tab, radius=1, min_arm=1)
        heads = np.arange(0, 2 * count, 2)
        assert (t["node"][heads] == 0).all() and (t["degree"][heads] == count).all()
        if count == 8:
            assert t["next"][heads].tolist() == heads[1:].tolist() + [0] and (t["flags"][heads] == M.MUTUAL).all()
            assert t["partner"][heads].tolist() == [8, 10, 12, 14, 0, 2, 4, 6] and (t["cos"][heads] == 1.0).all()
        else:
            assert (t["flags"][heads] == M.CROWDED).all() and (t["next"][heads] == -1).all() and (t["partner"][heads] == -1).all()
            assert (_bits(t["cos"][heads]) == M.QNAN_BITS).all() and (_bits(t["sin"][heads]) == M.QNAN_BITS).all() and (t["n"][heads] == 1).all()
        assert (t["degree"][heads + 1] == 1).all()
    tab[:, 3] = np.arange(9) % 2                                                 # two planes: five and four ends at the pixel
    t = M.joins(pts, tab, radius=1, min_arm=1)
    assert t["degree"][heads].tolist() == [5, 4] * 4 + [5] and t["node"][heads].tolist() == [0, 2] * 4 + [0]
    assert all(tab[p // 2, 3] == tab[e // 2, 3] for e, p in enumerate(t["partner"]) if p >= 0)


# ---- random masks: the structure of the nodes ----
@pytest.mark.parametrize("density", [0.2, 0.35, 0.5, 0.7])
def test_model_random_masks(density):
    mask = (np.random.default_rng(int(100 * density)).random((64, 64)) < density).astype(F32)
    pts, chains = CM.chains(mask)
    t = M.joins(pts, chains, radius=8)
    live = np.nonzero(t["node"] >= 0)[0]
    assert len(live) > 20 and not (t["degree"][live] == 2).any() and t["degree"][live].max() <= 4 and t["degree"][live].min() >= 1
    assert (t["flags"][t["node"] < 0] == M.NONE).all()
    for e in live:                                                              # the rings of `next` close
        ring, f = [int(e)], int(t["next"][e])
        while f != e and len(ring) <= 8:
            ring.append(f)
            f = int(t["next"][f])
        assert f == e and len(ring) == t["degree"][e] and (t["node"][ring] == min(ring)).all() and (t["degree"][ring] == len(ring)).all(), e
        assert len({(int(pts[chains[r // 2, 0] + (chains[r // 2, 1] - 1) * (r % 2), 0]), int(pts[chains[r // 2, 0] + (chains[r // 2, 1] - 1) * (r % 2), 1]))
                    for r in ring}) == 1                                         # one pixel
    mutual = np.nonzero(t["flags"] & M.MUTUAL)[0]
    assert len(mutual) >= 2 and len(mutual) % 2 == 0
    for e in mutual:                                                            # pairs, the same cosine, the opposite sine
        p = t["partner"][e]
        assert p != e and t["partner"][p] == e and t["flags"][p] & M.MUTUAL
        assert _bits(t["cos"][e]) == _bits(t["cos"][p]) and _bits(t["sin"][e]) ^ _bits(t["sin"][p]) == 0x80000000, e
    seen = set()
    for e in live[t["degree"][live] == 1]:                                      # from every free end: no end twice
        path = M.walk_mutual(t, e)
        assert len(path) == len(set(path)), e
        seen.update(path)
    assert seen


# ---- the ridge that turns by 120 degrees: the corner the turns cannot see ----
def test_model_ridge_of_120_degrees():
    """Thinning cuts the ridge at its vertex: three chains meet at one pixel, the two long arms and a three-point spur.  With min_arm = 3
    the spur's ends are SHORT and the two long chains are MUTUAL partners there; with min_arm = 1 the spur takes the join (cos 1.0 seen
    from the spur): this is why min_arm exists.  The cosine of the mutual join on the integer points, as this model measures it (printed):
        radius 4: -0.40614     radius 8: -0.43475     radius 16: -0.45754      (a turn by 120 degrees has cos -0.5)"""
    img, theta, (vx, vy), mask = TM.ridge_case(0.0, 120.0)
    pts, chains = CM.chains(mask)
    assert len(chains) == 3 and sorted(chains[:, 1].tolist())[0] == 3
    spur = int(np.argmin(chains[:, 1]))
    long_ = [c for c in range(3) if c != spur]
    t = M.joins(pts, chains, radius=8, min_arm=3, min_cos=-1.0)
    at = np.nonzero(t["degree"] == 3)[0]
    assert len(at) == 3 and sorted(a // 2 for a in at) == [0, 1, 2]
    vertex = pts[chains[at[0] // 2, 0] + (chains[at[0] // 2, 1] - 1) * (at[0] % 2)]
    assert np.hypot(vertex[0] - vx, vertex[1] - vy) <= 1.5                       # the node is the vertex pixel
    e, f = [a for a in at if a // 2 in long_]
    assert t["partner"][e] == f and t["partner"][f] == e and t["flags"][e] == t["flags"][f] == M.MUTUAL
    assert (t["flags"][[2 * spur, 2 * spur + 1]] == M.SHORT).all() and (t["partner"][[2 * spur, 2 * spur + 1]] == -1).all()
    assert -0.6 < t["cos"][e] < -0.3                                              # a turn by about 120 degrees
    for radius in (4, 8, 16):
        r = M.joins(pts, chains, radius=radius, min_arm=3)
        assert r["partner"][e] == f and r["flags"][e] & M.MUTUAL
        print("ridge of 120 degrees, radius %d: cos %.5f sin %.5f" % (radius, r["cos"][e], r["sin"][e]))
    greedy = M.joins(pts, chains, radius=8, min_arm=1)
    s = [a for a in at if a // 2 == spur][0]
    assert greedy["flags"][s] & M.MUTUAL and greedy["partner"][s] in (e, f)     # the spur steals the join
    assert not (greedy["flags"][e] & M.MUTUAL and greedy["flags"][f] & M.MUTUAL)
