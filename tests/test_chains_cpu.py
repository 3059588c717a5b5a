"""Contour chains (cvs_contour_chains) at every layer that exists without a GPU: the public header, the exports of both libraries, the Python
surface, the generated code of the new kernels (no scratch), and the Python model the GPU tests hold the kernels against -- its own
invariants on random masks, and hand cases with the expected lists written out."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import chains_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "cvsteer_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def test_header_declares_the_call_and_the_struct(tmp_path):
    text = open(os.path.join(ROOT, "include", "cvsteer_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int cvs_contour_chains\(cvs_handle h, const cvs_plane\* mask,\s*int32_t\* points, int point_capacity,\s*"
                     r"cvs_chain\* chains, int chain_capacity,\s*int mem,\s*int\* n_points, int\* n_chains\);", plain)
    assert re.search(r"#define CVS_ABI_VERSION 2\b", text)
    src = os.path.join(str(tmp_path), "layout.cpp")
    with open(src, "w") as f:
        f.write('#include <stddef.h>\n#include "cvsteer_hip.h"\n'
                'static_assert(sizeof(cvs_chain) == 16, "16 bytes");\n'
                'static_assert(offsetof(cvs_chain, start) == 0 && offsetof(cvs_chain, length) == 4, "start, length");\n'
                'static_assert(offsetof(cvs_chain, flags) == 8 && offsetof(cvs_chain, reserved) == 12, "flags, reserved");\n'
                'static_assert(CVS_CHAIN_CLOSED == 1 && CVS_CHAIN_HEAD_JUNCTION == 2 && CVS_CHAIN_TAIL_JUNCTION == 4, "flags");\n'
                'int main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), src], check=True)


def test_libraries_export_and_bind():
    import cvsteer_amd
    from cvsteer_amd import _lib as L
    assert L.SIGNATURES["cvs_contour_chains"] == (C.c_int, [C.c_void_p, L._PP, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, L._IP, L._IP])
    assert C.sizeof(L.Chain) == 16
    assert (cvsteer_amd.CHAIN_CLOSED, cvsteer_amd.CHAIN_HEAD_JUNCTION, cvsteer_amd.CHAIN_TAIL_JUNCTION) == (1, 2, 4)
    assert (M.CLOSED, M.HEAD_JUNCTION, M.TAIL_JUNCTION) == (1, 2, 4)
    hip = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "cvsteer_amd", "libcvsteer_hip.so")], text=True)
    assert re.search(r" T cvs_contour_chains$", hip, re.M)
    so = os.path.join(ROOT, "cvsteer_amd", "libcvsteer.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cvsteer_amd", "facade"), "-s"])
    syms = subprocess.check_output(["nm", "-DC", "--defined-only", so], text=True)
    for cls in ("SteerableFiltersG2", "SteerableFiltersG4"):
        assert re.search(r" T fa::%s::traceContours\(fa::Mat1f const&, std::vector<std::vector<fa::Point," % cls, syms), cls
    for cls in (cvsteer_amd.SteerableFiltersG2, cvsteer_amd.SteerableFiltersG4):
        assert callable(getattr(cls, "contour_chains", None))


def test_null_handle():
    from cvsteer_amd import _lib as L
    plane = L.Plane()
    n, m = C.c_int(-5), C.c_int(-6)
    assert L.lib().cvs_contour_chains(None, C.byref(plane), None, 0, None, 0, L.MEM_HOST, C.byref(n), C.byref(m)) == L.E_BADARG
    assert (n.value, m.value) == (-5, -6)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_chain_kernels_use_no_scratch(tmp_path):
    path = os.path.join(str(tmp_path), "cvs_kernels_chains.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    "-I" + SRC, "-S", "--cuda-device-only", os.path.join(SRC, "cvs_kernels_chains.hip"), "-o", path], check=True,
                   stderr=subprocess.DEVNULL)
    text = open(path).read()
    scratch = {}
    for blk in text.split("  - .agpr_count:")[1:]:
        nm = re.search(r"\.name:\s+(\S+)", blk)
        ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        if nm and ps:
            scratch[nm.group(1)] = int(ps.group(1))
    for stem in ("k_ch_links", "k_ch_nodes", "k_ch_roots", "k_ch_arc_count", "k_ch_arc_base", "k_ch_arcs", "k_ch_jump", "k_ch_heads",
                 "k_ch_head_count", "k_ch_head_apply", "k_ch_emit"):
        assert any(stem in n for n in scratch), (stem, sorted(scratch))
    assert len(scratch) == 11 and all(v == 0 for v in scratch.values()), scratch


# ---- the model against the contract's own consequences ----
def _lin(pts, cols):
    return (pts[:, 1].astype(np.int64) * cols + pts[:, 0]).tolist()


def _check_invariants(mask):
    rows, cols = mask.shape
    fg = M.foreground(mask)
    listed, adj = M.trace(mask)
    pts, table = M.chains(mask)
    nfg = int(fg.sum())
    deg = {p: len(v) for p, v in adj.items()}
    assert all(d <= 4 for d in deg.values())
    all_links = {(p, q) for p, v in adj.items() for q in v if p < q}
    assert all((q, p) not in all_links and p in adj[q] for p, q in all_links)          # symmetric
    covered = []
    for (path, flags), (start, length, tflags, zero) in zip(listed, table.tolist()):
        assert length == len(path) >= 1 and tflags == flags and zero == 0
        assert _lin(pts[start:start + length], cols) == path
        steps = list(zip(path[:-1], path[1:])) + ([(path[-1], path[0])] if flags & M.CLOSED else [])
        for p, q in steps:
            assert q in adj[p]
            assert max(abs(p // cols - q // cols), abs(p % cols - q % cols)) == 1     # 8-adjacent
            covered.append((min(p, q), max(p, q)))
        if flags & M.CLOSED:
            assert flags == M.CLOSED and all(deg[p] == 2 for p in path) and path[0] == min(path) and path[1] == adj[path[0]][0]
        elif len(path) == 1:
            assert flags == 0 and deg[path[0]] == 0
        else:
            assert all(deg[p] == 2 for p in path[1:-1]) and deg[path[0]] != 2 and deg[path[-1]] != 2
            assert (path[0], path[1]) != (path[-1], path[-2])                           # the two direction keys never tie
            assert (path[0], path[1]) < (path[-1], path[-2])
            assert bool(flags & M.HEAD_JUNCTION) == (deg[path[0]] >= 3) and bool(flags & M.TAIL_JUNCTION) == (deg[path[-1]] >= 3)
    assert sorted(covered) == sorted(all_links)                                         # every link exactly once
    assert set(_lin(pts, cols)) == set(np.flatnonzero(fg).tolist())                     # the union of the points is the foreground
    keys = [(path[0], path[1] if len(path) > 1 else -1) for path, _ in listed]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert table[:, 0].tolist() == np.concatenate([[0], np.cumsum(table[:, 1])[:-1]]).astype(int).tolist() if len(table) else True
    assert len(pts) <= 4 * nfg
    # the counts from degrees and components alone
    n_open = sum(d for d in deg.values() if d != 2) // 2
    n_iso = sum(1 for d in deg.values() if d == 0)
    seen, n_closed = set(), 0
    for p in sorted(adj):                                   # components of the link graph
        if p in seen:
            continue
        comp, stack = [], [p]
        seen.add(p)
        while stack:
            q = stack.pop()
            comp.append(q)
            for r in adj[q]:
                if r not in seen:
                    seen.add(r)
                    stack.append(r)
        n_closed += all(deg[q] == 2 for q in comp)
    assert len(table) == n_open + n_closed + n_iso
    assert len(pts) == len(all_links) + n_open + n_iso
    return len(table)


def test_model_invariants_on_random_masks():
    rng = np.random.default_rng(2024)
    chains = 0
    for density in (0.03, 0.1, 0.3, 0.5, 0.8, 1.0):
        for _ in range(34):
            shape = tuple(int(v) for v in rng.integers(1, 25, 2))
            chains += _check_invariants((rng.random(shape) < density).astype(np.float32))
    assert chains > 1000


def test_link_components_are_the_8_connected_components():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(5)
    for density in (0.1, 0.3, 0.5, 0.8):
        m = (rng.random((24, 24)) < density).astype(np.float32)
        lab, n = ndimage.label(m > 0, structure=np.ones((3, 3)))
        adj = M.adjacency(m)
        for p, v in adj.items():
            assert all(lab.flat[p] == lab.flat[q] for q in v)
        # and no finer: a union-find over the links finds n components
        parent = {p: p for p in adj}

        def find(p):
            while parent[p] != p:
                p = parent[p]
            return p
        for p, v in adj.items():
            for q in v:
                parent[find(p)] = find(q)
        assert len({find(p) for p in adj}) == n


# ---- hand cases, the expected lists written out ----
def _lists(mask):
    cols = np.asarray(mask).shape[1]
    pts, table = M.chains(np.float32(mask))
    return [(_lin(pts[s:s + n], cols), f) for s, n, f, _ in table.tolist()]


def test_block_of_four_is_one_closed_chain():
    assert _lists([[1, 1], [1, 1]]) == [([0, 1, 3, 2], M.CLOSED)]


def test_ring_goes_right_from_its_top_left_pixel():
    m = np.zeros((5, 5), np.float32)
    m[0, :] = m[4, :] = m[:, 0] = m[:, 4] = 1
    assert _lists(m) == [([0, 1, 2, 3, 4, 9, 14, 19, 24, 23, 22, 21, 20, 15, 10, 5], M.CLOSED)]
    pts, table = M.chains(m)
    assert pts[:3].tolist() == [[0, 0], [1, 0], [2, 0]] and table.tolist() == [[0, 16, 1, 0]]


def test_figure_eight_is_three_open_chains_between_two_junctions():
    m = np.float32([[1, 1, 1, 1, 1],
                    [1, 0, 0, 0, 1],
                    [1, 1, 1, 1, 1],
                    [1, 0, 0, 0, 1],
                    [1, 1, 1, 1, 1]])
    both = M.HEAD_JUNCTION | M.TAIL_JUNCTION
    assert _lists(m) == [([10, 5, 0, 1, 2, 3, 4, 9, 14], both),
                         ([10, 11, 12, 13, 14], both),
                         ([10, 15, 20, 21, 22, 23, 24, 19, 14], both)]


def test_t_shape():
    m = np.float32([[1, 1, 1, 1, 1],
                    [0, 0, 1, 0, 0],
                    [0, 0, 1, 0, 0]])
    assert _lists(m) == [([0, 1, 2], M.TAIL_JUNCTION),
                         ([2, 3, 4], M.HEAD_JUNCTION),
                         ([2, 7, 12], M.HEAD_JUNCTION)]


def test_single_pixel_and_empty_mask():
    assert _lists([[0, 0, 0], [0, 1, 0]]) == [([4], 0)]
    pts, table = M.chains(np.zeros((3, 4), np.float32))
    assert pts.shape == (0, 2) and table.shape == (0, 4) and pts.dtype == np.int32 and table.dtype == np.int32


def test_staircase_diagonal_is_no_link_and_a_bare_diagonal_is():
    assert _lists([[1, 1], [0, 1]]) == [([0, 1, 3], 0)]                      # 0 - 3 is the redundant diagonal of the corner
    assert _lists([[1, 0], [0, 1]]) == [([0, 3], 0)]
    assert _lists(np.uint8([[0, 7], [9, 0]])) == [([1, 2], 0)]
