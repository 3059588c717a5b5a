"""Test infrastructure (numpy and torch, no GPU needed to import): caller-owned planes as ROI views of sentinel-filled parents.

include/cvsteer_hip.h, "Conventions": a call writes exactly rows x cols elements of each output plane and not one byte more; it never
writes to an input; what lies around an input view never changes a result.  A PARENT is a buffer filled with a sentinel; a view inside it
is what the call is given.  Everything of the parent that no view owns -- the padding of every row, the rows above and below, the gutters
between views that lie side by side -- is the FRAME.  Sentinels are compared as bits, never as values:
    f32    a quiet NaN with a fixed payload (an output may hold NaN of its own; the frame must keep this exact pattern)
    u8     0xA5
    int32  0x5A5A5A5A

The three checks:
    assert_frame_intact(parent)     every element outside the views still holds its sentinel
    assert_inputs_intact(parent)    an input parent, view included, is bit for bit what it was before the call
    assert_same_bits(got, want)     the read footprint: the surroundings of an f32 input view hold the NaN sentinel, so a neighbour read into
                                    a sum shows even under a zero tap, and the call's outputs must equal those of the same call on a dense
                                    copy of the view; bytes have no NaN, so a byte input runs twice, surroundings 0x00 and 0xFF (BYTE_SURROUNDS)

tests/test_roi_guard_cpu.py proves these on a numpy surrogate kernel with one-line faults; tests/test_gpu_roi_footprint.py applies them to
every entry point of COVERED.  COVERED and EXEMPT together are the coverage ledger: every cvs_* function of the header whose parameter list
mentions cvs_plane or a capacity is on exactly one of the two.
"""
import re

import numpy as np

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

F32_SENTINEL_BITS = 0x7FC5A5A5      # quiet NaN, payload 0x05A5A5
U8_SENTINEL = 0xA5
S32_SENTINEL = 0x5A5A5A5A
BYTE_SURROUNDS = (0x00, 0xFF)

# name -> (rows above, rows below, elements left, elements right); "q" = one 16-byte unit of the plane's element type
PLACEMENTS = ("aligned", "odd", "tight", "wide", "side")
BYTE_PLACEMENTS = ("off1", "off2", "off3")      # byte planes, additionally: the packed byte stores
ALL_PLACEMENTS = PLACEMENTS + BYTE_PLACEMENTS


def _bits_dtype(dtype):
    return {1: np.uint8, 4: np.uint32, 8: np.uint64}[np.dtype(dtype).itemsize]


def sentinel_bits(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return F32_SENTINEL_BITS
    if dtype == np.uint8:
        return U8_SENTINEL
    if dtype == np.int32:
        return S32_SENTINEL
    raise ValueError("planes are float32, uint8 or int32, not %s" % dtype)


def margins(placement, cols, dtype):
    """(top, bottom, left, right) of a view of `cols` elements in its parent"""
    esz = np.dtype(dtype).itemsize
    if placement == "aligned":      # 16-byte start, pitch a multiple of 16 bytes (4 f32 elements): the float4 routes where cols % 4 == 0
        q = 16 // esz
        return 2, 3, q, q + (-cols % q)
    if placement == "odd":          # odd pitch: the dword routes
        right = 5 + ((cols + 8) % 2 == 0)
        return 1, 2, 3, right
    if placement == "tight":        # the smallest step that still has a frame
        return 1, 1, 0, 1
    if placement == "wide":         # a whole stray wave tile, strip or 32-row tile stays inside the parent
        return 32, 32, 64, 64
    if placement == "side":         # column windows of ONE parent, a one-element gutter between them (see windows())
        return 1, 1, 1, 1
    if placement == "dense":        # no frame at all (an input that is remembered, not surrounded)
        return 0, 0, 0, 0
    if placement in BYTE_PLACEMENTS:
        k = int(placement[3])
        if esz != 1:                # the f32 / int32 planes of a call with byte planes
            return 1, 2, 3, 5 + ((cols + 8) % 2 == 0)
        return 1, 1, k, 3
    raise ValueError("unknown placement %r" % (placement,))


def _aligned_empty(nbytes, align=64):
    raw = np.empty(nbytes + align, np.uint8)
    off = (-raw.ctypes.data) % align
    return raw[off:off + nbytes]


class Parent:
    """A sentinel-filled buffer (numpy, or a torch tensor on `device`) and the views handed out of it."""

    def __init__(self, shape, dtype, device=None, fill_bits=None):
        self.dtype = np.dtype(dtype)
        self.shape = tuple(int(v) for v in shape)
        self.sentinel = sentinel_bits(self.dtype) if fill_bits is None else int(fill_bits)
        n = int(np.prod(self.shape))
        host = _aligned_empty(n * self.dtype.itemsize).view(_bits_dtype(self.dtype)).reshape(self.shape)
        host[...] = self.sentinel
        host = host.view(self.dtype)
        self.device = device
        self.buf = host if device is None else torch.from_numpy(host).to(device)
        self.owned = np.zeros(self.shape, bool)
        self.windows = []
        self.before = None

    def claim(self, idx):
        """the view buf[idx]; its elements leave the frame"""
        if self.owned[idx].any():
            raise ValueError("views of one parent share nothing")
        self.owned[idx] = True
        self.windows.append(idx)
        return self.buf[idx]

    def bits(self):
        a = self.buf if self.device is None else self.buf.cpu().numpy()
        return np.ascontiguousarray(a).view(_bits_dtype(self.dtype))

    def snapshot(self):
        self.before = self.bits().copy()

    def origin(self):
        """parent index of the first element of the first view"""
        idx = self.windows[0] if self.windows else ()
        return tuple((s.start or 0) if isinstance(s, slice) else int(s) for s in idx) + (0,) * (len(self.shape) - len(idx))


def window(shape, dtype, placement, device=None, fill_bits=None):
    """(parent, view): one rows x cols view placed as `placement` says"""
    rows, cols = shape
    t, b, l, r = margins(placement, cols, dtype)
    p = Parent((rows + t + b, cols + l + r), dtype, device, fill_bits)
    return p, p.claim((slice(t, t + rows), slice(l, l + cols)))


def windows(specs, placement, device=None):
    """Output planes for one call.  specs: [(shape, dtype), ...].  Returns (parents, views), views in the order of specs.  Every placement
    but "side" gives each plane a parent of its own; "side" puts all planes of one dtype and height into ONE parent as column windows
    with a one-element gutter between them."""
    views, parents = [None] * len(specs), []
    if placement != "side":
        for i, (shape, dtype) in enumerate(specs):
            p, views[i] = window(shape, dtype, placement, device)
            parents.append(p)
        return parents, views
    groups = {}
    for i, (shape, dtype) in enumerate(specs):
        groups.setdefault((np.dtype(dtype).str, shape[0]), []).append(i)
    for (dt, rows), members in groups.items():
        t, b, l, r = margins("side", 0, dt)
        width = l + sum(specs[i][0][1] + 1 for i in members) - 1 + r
        p = Parent((rows + t + b, width), dt, device)
        c = l
        for i in members:
            cols = specs[i][0][1]
            views[i] = p.claim((slice(t, t + rows), slice(c, c + cols)))
            c += cols + 1
        parents.append(p)
    return parents, views


def block(shape, haxis, placement, dtype=np.float32, device=None):
    """(parent, inner): an N-D block of planes -- [N][K][H][W], [H][K][W], ... -- whose last axis W is a column slice of a wider parent and
    whose axis `haxis` has guard rows above and below.  `inner` has `shape`; index it to get the planes."""
    shape = tuple(shape)
    t, b, l, r = margins(placement, shape[-1], dtype)
    big = list(shape)
    big[haxis] += t + b
    big[-1] += l + r
    p = Parent(big, dtype, device)
    idx = [slice(None)] * len(shape)
    idx[haxis] = slice(t, t + shape[haxis])
    idx[-1] = slice(l, l + shape[-1])
    return p, p.claim(tuple(idx))


def array(n, dtype, front, back, device=None):
    """(parent, view): an array of n elements (n may be a shape whose first axis is the list axis) as a slice of a longer sentinel
    buffer, `front` elements guarded in front of it and `back` behind it"""
    tail = tuple(n[1:]) if isinstance(n, (tuple, list)) else ()
    n0 = int(n[0]) if isinstance(n, (tuple, list)) else int(n)
    p = Parent((front + n0 + back,) + tail, dtype, device)
    return p, p.claim((slice(front, front + n0),))


def _finish_input(host, idx, values, device):
    host.claim(idx)[...] = values
    if device is not None:
        host.device = device
        host.buf = torch.from_numpy(host.buf).to(device)
    host.snapshot()
    return host, host.buf[idx]


def guard_input(values, placement, device=None, surround=None, haxis=None):
    """(parent, view): `values` (numpy; 2-D, or an N-D block of planes whose row axis is `haxis`) as a view whose surroundings hold the
    sentinel -- or the byte `surround` (BYTE_SURROUNDS); the parent's bits are remembered for assert_inputs_intact"""
    values = np.ascontiguousarray(values)
    haxis = values.ndim - 2 if haxis is None else haxis
    t, b, l, r = margins(placement, values.shape[-1], values.dtype)
    big = list(values.shape)
    big[haxis] += t + b
    big[-1] += l + r
    idx = [slice(None)] * values.ndim
    idx[haxis] = slice(t, t + values.shape[haxis])
    idx[-1] = slice(l, l + values.shape[-1])
    return _finish_input(Parent(big, values.dtype, None, surround), tuple(idx), values, device)


def guard_input_array(values, front, back, device=None):
    """(parent, view): an input array (first axis = the list axis) as a slice of a longer sentinel buffer, remembered like guard_input's"""
    values = np.ascontiguousarray(values)
    host = Parent((front + len(values) + back,) + values.shape[1:], values.dtype)
    return _finish_input(host, (slice(front, front + len(values)),), values, device)


# ---------------------------------------------------------------- the checks
def assert_frame_intact(parent, name=""):
    bits = parent.bits()
    bad = (bits != bits.dtype.type(parent.sentinel)) & ~parent.owned
    if bad.any():
        where = np.argwhere(bad)
        first = tuple(int(a) - int(o) for a, o in zip(where[0], parent.origin()))
        raise AssertionError("%s: %d element(s) outside the view(s) were written; the first at (row, column) = %s relative to the first view, "
                             "now 0x%X (sentinel 0x%X); parent %s %s" % (name or "frame", len(where), first[-2:] if len(first) >= 2 else first,
                                                                         int(bits[tuple(where[0])]), parent.sentinel, parent.shape, parent.dtype))


def assert_inputs_intact(parent, name=""):
    if parent.before is None:
        raise ValueError("no snapshot: make input parents with guard_input()")
    now = parent.bits()
    bad = now != parent.before
    if bad.any():
        where = np.argwhere(bad)
        first = tuple(int(a) - int(o) for a, o in zip(where[0], parent.origin()))
        raise AssertionError("%s: the call changed %d element(s) of an input parent; the first at (row, column) = %s relative to the view"
                             % (name or "input", len(where), first[-2:] if len(first) >= 2 else first))


def to_numpy(a):
    if torch is not None and isinstance(a, torch.Tensor):
        return a.detach().cpu().numpy()
    return np.asarray(a)


def assert_same_bits(got, want, name=""):
    """two lists of arrays, bit for bit (NaN payloads included)"""
    assert len(got) == len(want), (name, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.ascontiguousarray(to_numpy(g)), np.ascontiguousarray(to_numpy(w))
        assert g.shape == w.shape and g.dtype == w.dtype, "%s: result %d is %s %s, the dense call's %s %s" % (name, k, g.shape, g.dtype, w.shape, w.dtype)
        if g.tobytes() != w.tobytes():
            gb, wb = g.view(_bits_dtype(g.dtype) if g.dtype.names is None else np.uint8), w.view(_bits_dtype(w.dtype) if w.dtype.names is None else np.uint8)
            where = np.argwhere(gb != wb)
            sent = int((gb == gb.dtype.type(sentinel_bits(g.dtype))).sum()) if g.dtype in (np.float32, np.uint8, np.int32) else 0
            raise AssertionError("%s: result %d differs from the dense call's in %d of %d elements, the first at %s (%d of its elements hold the "
                                 "sentinel)" % (name, k, len(where), gb.size, tuple(int(v) for v in where[0]), sent))


# ---------------------------------------------------------------- the coverage ledger
# entry points tests/test_gpu_roi_footprint.py drives through the guard (its table is generated from this list: a name without a row fails
# at collection)
COVERED = [
    "cvs_setup_steer", "cvs_read_state", "cvs_steer_scalar", "cvs_steer_map", "cvs_steer_bank", "cvs_orientation_peaks", "cvs_mag_phase",
    "cvs_wrap", "cvs_phase_weights", "cvs_find", "cvs_nonmax", "cvs_hysteresis", "cvs_label", "cvs_component_stats", "cvs_contour_prune",
    "cvs_contour_points", "cvs_contour_chains", "cvs_chain_polylines", "cvs_chain_refine", "cvs_link", "cvs_nonmax_batch",
    "cvs_contours_batch", "cvs_contour_chains_batch", "cvs_chain_refine_batch", "cvs_pipeline", "cvs_pipeline_batch", "cvs_pyr_down",
    "cvs_setup_pyr", "cvs_pyramid_setup",
]
EXEMPT = {
    "cvs_setup": "reads its image plane only; its outputs are the handle's own state planes",
    "cvs_setup_rows": "reads its image plane only; its outputs are the handle's own state planes",
    "cvs_state_plane": "hands out a view of a state plane; nothing is written",
    "cvs_normalize_u8": "row padding of the destination already guarded in test_gpu_u8_reference.py",
    "cvs_convert_u8": "row padding of the destination already guarded in test_gpu_u8_reference.py",
    "cvs_normalize_u8_batch": "row padding of the destinations already guarded in test_gpu_u8_reference.py",
    "cvs_convert_u8_batch": "row padding of the destinations already guarded in test_gpu_u8_reference.py",
    "cvs_batch_run": "batch layer: the padding of its host rows is guarded in test_gpu_batch.py",
    "cvs_batch_pyramid_setup": "batch layer: reads the root's image plane only",
    "cvs_batch_level": "hands out a handle and a view of a level image; nothing is written",
}


def header_entry_points(text):
    """the cvs_* functions declared in the header text whose parameter list mentions cvs_plane or a capacity"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = set()
    for m in re.finditer(r"\b(?:int|const\s+char\s*\*)\s+(cvs_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        if re.search(r"\bcvs_plane\b|capacity", m.group(2)):
            out.add(m.group(1))
    return out
