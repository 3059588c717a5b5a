"""Host-side mirror of the reference's class surface (namespace fa) over the C ABI.

Reference: cvsteer/SteerableFilters.h:41-50, SteerableFiltersG2.h:35-67,
SteerableFiltersG4.h:35-57.  Method names and argument meaning follow the reference; where the
reference fills ``cv::Mat1f&`` out-parameters, these methods return the planes.

Planes may be
  * numpy float32 arrays (host memory; results come back as numpy arrays), or
  * torch CUDA float32 tensors (device memory; zero-copy in, results are torch tensors on the
    same device, work is enqueued on torch's current stream).
All arithmetic happens in libcvsteer_hip.so on the GPU; this module only marshals pointers.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from ._lib import CvsError, Plane, lib

SETUP_BASIS, SETUP_ORIENT, SETUP_FULL = 1, 2, 3

try:  # torch is plumbing (device memory + streams), optional for host-plane use
    import torch
except Exception:  # pragma: no cover
    torch = None


# numpy mirror of `struct cvs_plane` (include/cvsteer_hip.h) for arrays of descriptors
_PLANE_DTYPE = np.dtype({"names": ["data", "rows", "cols", "step", "mem"], "formats": ["u8", "i4", "i4", "u8", "i4"],
                         "offsets": [Plane.data.offset, Plane.rows.offset, Plane.cols.offset, Plane.step.offset, Plane.mem.offset],
                         "itemsize": C.sizeof(Plane)})


def _is_torch(a):
    return torch is not None and isinstance(a, torch.Tensor)


KIND_G2, KIND_G4 = L.KIND_G2, L.KIND_G4
CHAIN_CLOSED, CHAIN_HEAD_JUNCTION, CHAIN_TAIL_JUNCTION = L.CHAIN_CLOSED, L.CHAIN_HEAD_JUNCTION, L.CHAIN_TAIL_JUNCTION
# numpy mirror of `struct cvs_chain_bridge`: one record per chain end
BRIDGE_DTYPE = np.dtype([("partner", "<i4"), ("flags", "<i4"), ("n", "<i4"), ("steps", "<i4"), ("bridge", "<i4"), ("start", "<i4"), ("cos", "<f4"),
                         ("cos_partner", "<f4")])


def alloc_planes(n, rows, cols, device=None):
    """n output planes as rows of ONE block, [row][plane][column] -- the layout the engine gives its own state planes
    (CVS_OPT_STATE_LAYOUT): a launch that writes all of them streams one linear sweep instead of n streams far apart.
    Returns n strided (rows, cols) views, ordinary planes for every entry point (like cv::Mat ROIs: step = n * cols * 4).
    device=None: numpy (host) planes."""
    if device is None:
        blk = np.empty((rows, n, cols), np.float32)
    else:
        blk = torch.empty((rows, n, cols), dtype=torch.float32, device=device)
    return [blk[:, k, :] for k in range(n)]


def num_basis(kind):
    return lib().cvs_num_basis(kind)


def make_taps(kind, idx, width, spacing):
    """SteerableFilters::create on the idx-th tap function (host math, no GPU needed)."""
    out = np.empty(2 * width + 1, np.float32)
    rc = lib().cvs_make_taps(kind, idx, width, spacing, out.ctypes.data_as(C.POINTER(C.c_float)))
    if rc:
        raise CvsError(rc, "cvs_make_taps")
    return out


def basis_taps(kind, p):
    a, b = C.c_int(), C.c_int()
    rc = lib().cvs_basis_taps(kind, p, C.byref(a), C.byref(b))
    if rc:
        raise CvsError(rc, "cvs_basis_taps")
    return a.value, b.value


def steer_weights(kind, theta):
    out = np.empty(num_basis(kind), np.float32)
    rc = lib().cvs_steer_weights(kind, theta, out.ctypes.data_as(C.POINTER(C.c_float)))
    if rc:
        raise CvsError(rc, "cvs_steer_weights")
    return out


def _plane(a):
    """cvs_plane view of a 2-D float32 numpy array or torch CUDA tensor (no copy); 8-bit arrays /
    tensors are accepted for input images (CVS_DEPTH_U8), int32 ones for label planes (CVS_DEPTH_S32)."""
    if (_is_torch(a) and a.dtype == torch.int32) or (isinstance(a, np.ndarray) and a.dtype == np.int32):
        t = _is_torch(a)
        if a.ndim != 2 or ((a.numel() if t else a.size) and a.shape[1] > 1 and (a.stride(1) != 1 if t else a.strides[1] != 4)):
            raise ValueError("label plane must be 2-D int32 with unit column stride")
        mem = (L.MEM_DEVICE if (t and a.is_cuda) else L.MEM_HOST) | L.DEPTH_S32
        step = (a.stride(0) * 4 if t else a.strides[0]) if (a.shape[0] > 1 and a.shape[1] > 0) else a.shape[1] * 4
        return Plane(a.data_ptr() if t else a.ctypes.data, a.shape[0], a.shape[1], step, mem)
    if _is_torch(a) and a.dtype == torch.uint8:
        if a.dim() != 2 or (a.numel() and a.shape[1] > 1 and a.stride(1) != 1):
            raise ValueError("8-bit image must be 2-D with unit column stride")
        mem = (L.MEM_DEVICE if a.is_cuda else L.MEM_HOST) | L.DEPTH_U8
        return Plane(a.data_ptr(), a.shape[0], a.shape[1], a.stride(0) if a.shape[0] > 1 else a.shape[1], mem)
    if isinstance(a, np.ndarray) and a.dtype == np.uint8:
        if a.ndim != 2 or (a.size and a.shape[1] > 1 and a.strides[1] != 1):
            raise ValueError("8-bit image must be 2-D with unit column stride")
        return Plane(a.ctypes.data, a.shape[0], a.shape[1], a.strides[0] if (a.shape[0] > 1 and a.size) else a.shape[1],
                     L.MEM_HOST | L.DEPTH_U8)
    if _is_torch(a):
        if a.dtype != torch.float32 or a.dim() != 2 or (a.numel() and a.shape[1] > 1 and a.stride(1) != 1):
            raise ValueError("torch plane must be 2-D float32 with unit column stride")
        mem = L.MEM_DEVICE if a.is_cuda else L.MEM_HOST
        return Plane(a.data_ptr(), a.shape[0], a.shape[1], a.stride(0) * 4 if a.shape[0] > 1 else a.shape[1] * 4, mem)
    if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.ndim != 2:
        raise ValueError("numpy plane must be 2-D float32")
    if a.size and a.shape[1] > 1 and a.strides[1] != 4:
        raise ValueError("numpy plane must have unit column stride")
    step = a.strides[0] if (a.shape[0] > 1 and a.size) else a.shape[1] * 4
    return Plane(a.ctypes.data, a.shape[0], a.shape[1], step, L.MEM_HOST)


def _planes(seq):
    return (Plane * len(seq))(*[_plane(x) for x in seq])


def _as_input(a):
    """the reference converts any Mat to Mat1f unscaled (Mat1f(const Mat&)); do the same on the host side"""
    if _is_torch(a):
        return a if a.dtype in (torch.float32, torch.uint8) else a.to(torch.float32)
    a = np.asarray(a)
    return a if a.dtype in (np.float32, np.uint8) else a.astype(np.float32)


def pyramid_setup(handles, image, level_images=None, flags=SETUP_BASIS):
    """BASELINE config 3 in one call (cvs_pyramid_setup): handles[l].setup(level l) for every level of the Gaussian pyramid of
    `image`, the pyramid built on the way (the filter launch of a level writes the next level).  level_images: the levels - 1 planes that receive levels 1.. (allocated when None).
    Returns [image, level 1, ...]."""
    n = len(handles)
    image = _as_input(image)
    if level_images is None:
        level_images, shape = [], tuple(image.shape)
        for _ in range(n - 1):
            shape = ((shape[0] + 1) // 2, (shape[1] + 1) // 2)
            level_images.append(torch.empty(shape, dtype=torch.float32, device=image.device) if _is_torch(image) else np.empty(shape, np.float32))
    for hnd in handles:
        hnd._bind_stream(image, *level_images)
    arr = (C.c_void_p * n)(*[hnd._h for hnd in handles])
    planes = (Plane * max(1, n - 1))(*[_plane(l) for l in level_images])
    pi = _plane(image)
    rc = lib().cvs_pyramid_setup(arr, n, C.byref(pi), int(flags), planes)
    if rc:
        raise CvsError(rc, "cvs_pyramid_setup", lib().cvs_last_error(handles[0]._h).decode())
    for hnd, l in zip(handles, [image] + list(level_images)):
        hnd._like = l
        hnd._image_keepalive = l
    return [image] + list(level_images)


class SteerableFilters:
    """fa::SteerableFilters (SteerableFilters.h:41-50): setup(image), steer(theta) -> (g, h)."""

    KIND = None
    DEFAULT_WIDTH = None
    DEFAULT_SPACING = None

    def __init__(self, image=None, width=None, spacing=None, device=None, setup_flags=None):
        width = self.DEFAULT_WIDTH if width is None else width
        spacing = self.DEFAULT_SPACING if spacing is None else spacing
        if device is None:
            device = image.device.index if (_is_torch(image) and image.is_cuda and image.device.index is not None) else 0
        self._h = C.c_void_p()
        rc = lib().cvs_create(self.KIND, int(width), float(spacing), int(device), C.byref(self._h))
        if rc:
            self._h = None
            raise CvsError(rc, "cvs_create", "no usable HIP device -- there is no CPU fallback" if rc == L.E_HIP else "")
        self.device = int(device)
        self.width, self.spacing = int(width), float(spacing)
        self._like = None
        self._setup_flags = setup_flags
        if image is not None:
            self.setup(image)

    # -- plumbing --
    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                lib().cvs_destroy(h)
            except Exception:
                pass

    def _check(self, rc, where):
        if rc:
            raise CvsError(rc, where, lib().cvs_last_error(self._h).decode())

    def _bind_stream(self, *planes):
        if torch is not None and any(_is_torch(p) and p.is_cuda for p in planes):
            lib().cvs_set_stream(self._h, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))

    def _new(self, shape=None):
        shape = self.shape if shape is None else shape
        if _is_torch(self._like) and self._like.is_cuda:
            return torch.empty(shape, dtype=torch.float32, device=self._like.device)
        return np.empty(shape, np.float32)

    def _new_like(self, a):
        if _is_torch(a):
            return torch.empty(tuple(a.shape), dtype=torch.float32, device=a.device)
        return np.empty(a.shape, np.float32)

    def _new_block_like(self, a, n):
        """n fresh output planes shaped like `a`: device planes come as rows of one block (alloc_planes), host planes dense"""
        if _is_torch(a) and a.is_cuda:
            return alloc_planes(n, int(a.shape[0]), int(a.shape[1]), device=a.device)
        return [self._new_like(a) for _ in range(n)]

    def set_option(self, option, value):
        self._check(lib().cvs_set_option(self._h, option, int(value)), "cvs_set_option")

    def get_option(self, option):
        v = C.c_int(0)
        self._check(lib().cvs_get_option(self._h, option, C.byref(v)), "cvs_get_option")
        return v.value

    def launch_info(self):
        """cvs_get_launch_info as a dict: configuration of the last basis launch (the engine's default or its tuner's decision)"""
        li = L.LaunchInfo()
        li.struct_size = C.sizeof(L.LaunchInfo)
        self._check(lib().cvs_get_launch_info(self._h, C.byref(li)), "cvs_get_launch_info")
        return {k: getattr(li, k) for k, _ in L.LaunchInfo._fields_}

    def set_atan_mode(self, exact):
        self.set_option(L.OPT_ATAN_MODE, 1 if exact else 0)

    def set_strip_rows(self, rows):
        self.set_option(L.OPT_STRIP_ROWS, rows)

    def sync(self):
        self._check(lib().cvs_sync(self._h), "cvs_sync")

    @property
    def shape(self):
        r, c = C.c_int(), C.c_int()
        self._check(lib().cvs_shape(self._h, C.byref(r), C.byref(c)), "cvs_shape")
        return (r.value, c.value)

    def taps(self, idx):
        out = np.empty(2 * self.width + 1, np.float32)
        self._check(lib().cvs_taps(self._h, idx, out.ctypes.data_as(C.POINTER(C.c_float))), "cvs_taps")
        return out

    def _state(self, which):
        out = self._new()
        self._bind_stream(out)
        p = _plane(out)
        self._check(lib().cvs_read_state(self._h, which, C.byref(p)), "cvs_read_state")
        return out

    def basis(self, p):
        """p-th separable basis plane (the reference's protected m_g2a.. / m_g4a.. members)."""
        return self._state(L.PLANE_BASIS0 + p)

    def basis_view(self, p):
        """zero-copy (ptr, rows, cols, step_bytes) of a device-resident basis plane"""
        v = Plane()
        self._check(lib().cvs_state_plane(self._h, L.PLANE_BASIS0 + p, C.byref(v)), "cvs_state_plane")
        return v.data, v.rows, v.cols, v.step

    # -- reference surface --
    def setup(self, image, flags=None):
        """virtual setup(const Mat1f&)"""
        image = _as_input(image)
        if flags is None:
            flags = self._setup_flags if self._setup_flags is not None else self._DEFAULT_FLAGS
        self._like = image
        self._bind_stream(image)
        p = _plane(image)
        self._image_keepalive = image
        self._check(lib().cvs_setup(self._h, C.byref(p), flags), "cvs_setup")

    def setup_steer(self, image, theta, flags=SETUP_BASIS, out=None):
        """setup(image) + steer(float theta) in one kernel launch -> (g, h)"""
        image = _as_input(image)
        self._like = image
        g, h = out if out is not None else self._new_block_like(image, 2)
        self._bind_stream(image, g, h)
        pi, pg, ph = _plane(image), _plane(g), _plane(h)
        self._check(lib().cvs_setup_steer(self._h, C.byref(pi), flags, float(theta), C.byref(pg), C.byref(ph)),
                    "cvs_setup_steer")
        return g, h

    def _steer(self, theta, full, out=None):
        n = 5 if full else 2
        outs = list(out) if out is not None else [self._new() for _ in range(n)]
        planes = [_plane(o) for o in outs] + [None] * (5 - n)
        ptrs = [C.byref(p) if p is not None else None for p in planes]
        if isinstance(theta, (int, float, np.floating)):
            self._bind_stream(*outs)
            self._check(lib().cvs_steer_scalar(self._h, float(theta), *ptrs), "cvs_steer_scalar")
        else:
            if theta is not None:
                theta = _as_input(theta)
                self._bind_stream(theta, *outs)
                pt = _plane(theta)
                tptr = C.byref(pt)
            else:
                self._bind_stream(*outs)
                tptr = None
            self._check(lib().cvs_steer_map(self._h, tptr, *ptrs), "cvs_steer_map")
        return tuple(outs)

    def steer(self, theta, full=False, out=None):
        """steer(float theta, g, h) / steer(const Mat1f& theta, g, h); theta=None steers at the
        dominant orientation.  full=True adds (e, magnitude, phase) (G2 only)."""
        return self._steer(theta, full, out)

    def steer_bank(self, thetas, full=False, outputs=None, out=None):
        """steer(float theta, ...) at every angle of `thetas` (1-D) in one pass over the basis planes (cvs_steer_bank).
        outputs: indices into (g, h, e, magnitude, phase), default (0, 1); full=True = all five (G4: CVS_OPT_G4_EXTENSIONS).
        Returns one (K, H, W) array per requested kind, in that order, allocated as one block, or `out`: one (K, H, W) array or
        sequence of K planes per kind.  Plane k of each equals steer(thetas[k]) bit for bit."""
        if _is_torch(thetas):
            thetas = thetas.detach().cpu().numpy()
        th = np.ascontiguousarray(np.asarray(thetas, dtype=np.float32))
        if th.ndim != 1 or th.size == 0:
            raise ValueError("thetas must be a non-empty 1-D sequence of angles")
        kinds = (0, 1, 2, 3, 4) if full else ((0, 1) if outputs is None else tuple(int(o) for o in outputs))
        if not kinds or len(set(kinds)) != len(kinds) or any(o < 0 or o > 4 for o in kinds):
            raise ValueError("outputs: distinct indices into (g, h, e, magnitude, phase)")
        n = int(th.size)
        if out is None:
            blk = self._new((len(kinds), n) + tuple(self.shape))
            out = [blk[i] for i in range(len(kinds))]
        out = list(out)
        if len(out) != len(kinds):
            raise ValueError("out: one (K, H, W) array per requested kind")
        planes = (Plane * (5 * n))()   # zeroed: data == NULL = not written
        for o, arr in zip(kinds, out):
            if len(arr) != n:
                raise ValueError("out: each array holds one plane per angle")
            for k in range(n):
                planes[5 * k + o] = _plane(arr[k])
        self._bind_stream(*out)
        self._check(lib().cvs_steer_bank(self._h, th.ctypes.data_as(C.POINTER(C.c_float)), n, planes), "cvs_steer_bank")
        return tuple(out)

    def orientation_peaks(self, n_angles=16, max_peaks=2, min_energy=0.0, min_ratio=0.25, min_contrast=1e-3, out=None):
        """every local orientation of each pixel (cvs_orientation_peaks): the oriented energy g^2 + h^2 at n_angles angles k pi / K, its
        circular local maxima refined by a parabola, the max_peaks strongest kept -- one pass over the basis planes.
        Returns (angles[M, H, W], energies[M, H, W], count[H, W] uint8): slot 0 is the strongest peak, slots from count upward hold
        angle -1 and energy 0.  An angle theta is the steering angle: the direction across the structure is (cos theta, -sin theta)
        in (column, row) steps, so a ridge of direction phi peaks at phi + pi / 2 (mod pi).
        out: (angles, energies, count), any of them None = not written (and returned as None)."""
        M = int(max_peaks)
        if out is None:
            shape = tuple(self.shape)
            blk = self._new((2, M) + shape) if 1 <= M <= L.PEAKS_MAX else self._new((2, 1) + shape)   # (the library refuses M)
            cnt = torch.empty(shape, dtype=torch.uint8, device=blk.device) if _is_torch(blk) else np.empty(shape, np.uint8)
            out = (blk[0], blk[1], cnt)
        ang, en, cnt = out
        if ang is None and en is None and cnt is None:
            raise ValueError("out: at least one of (angles, energies, count)")
        if 1 <= M <= L.PEAKS_MAX and any(x is not None and len(x) != M for x in (ang, en)):
            raise ValueError("out: angles and energies hold max_peaks planes each")
        cfg = L.PeaksCfg(C.sizeof(L.PeaksCfg), int(n_angles), M, float(min_energy), float(min_ratio), float(min_contrast))
        pa = _planes(list(ang)) if ang is not None else None
        pe = _planes(list(en)) if en is not None else None
        pc = _plane(cnt) if cnt is not None else None
        self._bind_stream(*([] if ang is None else list(ang)), *([] if en is None else list(en)), cnt)
        self._check(lib().cvs_orientation_peaks(self._h, C.byref(cfg), pa, pe, C.byref(pc) if pc is not None else None),
                    "cvs_orientation_peaks")
        return ang, en, cnt

    # -- adjacent component: Gaussian pyramid, not part of the reference --
    def pyrDown(self, image):
        """one pyramid level with cv::pyrDown semantics: ((rows+1)//2, (cols+1)//2)"""
        image = _as_input(image)
        shape = ((image.shape[0] + 1) // 2, (image.shape[1] + 1) // 2)
        if _is_torch(image):
            dst = torch.empty(shape, dtype=torch.float32, device=image.device)
        else:
            dst = np.empty(shape, np.float32)
        self._bind_stream(image, dst)
        ps, pd = _plane(image), _plane(dst)
        self._check(lib().cvs_pyr_down(self._h, C.byref(ps), C.byref(pd)), "cvs_pyr_down")
        return dst

    def pyramid(self, image, levels):
        """[image, pyrDown(image), ...] -- `levels` planes"""
        out = [_as_input(image)]
        for _ in range(levels - 1):
            out.append(self.pyrDown(out[-1]))
        return out

    def setup_pyr(self, image, flags=None, out=None):
        """setup(image) and pyrDown(image) in one pass over the image -> the next pyramid level"""
        image = _as_input(image)
        if flags is None:
            flags = self._setup_flags if self._setup_flags is not None else self._DEFAULT_FLAGS
        shape = ((image.shape[0] + 1) // 2, (image.shape[1] + 1) // 2)
        if out is not None:
            dst = out
        elif _is_torch(image):
            dst = torch.empty(shape, dtype=torch.float32, device=image.device)
        else:
            dst = np.empty(shape, np.float32)
        self._like = image
        self._bind_stream(image, dst)
        self._image_keepalive = image
        ps, pd = _plane(image), _plane(dst)
        self._check(lib().cvs_setup_pyr(self._h, C.byref(ps), flags, C.byref(pd)), "cvs_setup_pyr")
        return dst


class _CallerPipeline:
    """The callers' sequence (test/test.cpp:85-90, example/steer.cpp:86-122) on a SteerableFilters object: find*, the fused
    pipeline for one image or a batch of frames, and the 8-bit conversions.  Shared by G2 and -- with extensions on -- G4."""

    def _caller_check(self, where):
        """raises CvsError(E_UNSUPPORTED) where the object has no caller pipeline"""

    def find(self, e, phase, which=(True, True, True)):
        """findEdges + findDarkLines + findBrightLines in one pass -> (edges, dark, bright)"""
        self._caller_check("cvs_find")
        outs = [self._new_like(e) if w else None for w in which]
        self._bind_stream(e, phase, *[o for o in outs if o is not None])
        pe, pp = _plane(e), _plane(phase)
        planes = [_plane(o) if o is not None else None for o in outs]
        ptrs = [C.byref(p) if p is not None else None for p in planes]
        self._check(lib().cvs_find(self._h, C.byref(pe), C.byref(pp), *ptrs), "cvs_find")
        return tuple(outs)

    def findEdges(self, e, phase, k=2.0):
        return self.find(e, phase, (True, False, False))[0]

    def findDarkLines(self, e, phase, k=2.0):
        return self.find(e, phase, (False, True, False))[1]

    def findBrightLines(self, e, phase, k=2.0):
        return self.find(e, phase, (False, False, True))[2]

    def _u8_dtype(self, dtype):
        """dtype=None / float32: f32 outputs; uint8 (torch or numpy): 8-bit outputs (set_u8_gain says how they are made)"""
        if dtype is None or dtype is np.float32 or (torch is not None and dtype is torch.float32) or dtype == np.float32:
            return False
        if dtype is np.uint8 or (torch is not None and dtype is torch.uint8) or dtype == np.uint8:
            return True
        raise ValueError("pipeline outputs are float32 or uint8, not %r" % (dtype,))

    def _new_u8_planes(self, like, n):
        if _is_torch(like) and like.is_cuda:
            return list(torch.empty((n,) + tuple(like.shape), dtype=torch.uint8, device=like.device))
        return [np.empty(like.shape, np.uint8) for _ in range(n)]

    def set_u8_gain(self, gain):
        """8-bit pipeline outputs: 0 (default) = normalize(0, 255, NORM_MINMAX, CV_8UC1) per map, > 0 = convertTo(CV_8UC1, gain)
        (example/steer.cpp:92-104); negative or NaN raises CvsError(E_BADARG)"""
        self._check(lib().cvs_set_u8_gain(self._h, float(gain)), "cvs_set_u8_gain")

    def u8_gain(self):
        v = C.c_float(0.0)
        self._check(lib().cvs_get_u8_gain(self._h, C.byref(v)), "cvs_get_u8_gain")
        return v.value

    def pipeline(self, image, out=None, dtype=None):
        """the callers' whole sequence (test/test.cpp:85-90) for one image ->
        (g, h, e, magnitude, phase, edges, dark, bright) -- g2 / h2, or g4 / h4.  uint8 `out` planes (or dtype=uint8) receive the maps as
        bytes, made as set_u8_gain says."""
        image = _as_input(image)
        self._like = image
        if out is not None:
            outs = list(out)
        elif self._u8_dtype(dtype):
            outs = self._new_u8_planes(image, 8)
        else:
            outs = self._new_block_like(image, 8)
        self._bind_stream(image, *[o for o in outs if o is not None])
        pi = _plane(image)
        planes = [_plane(o) if o is not None else None for o in outs]
        arr = (C.POINTER(Plane) * 8)(*[C.pointer(p) if p is not None else None for p in planes])
        self._check(lib().cvs_pipeline(self._h, C.byref(pi), arr), "cvs_pipeline")
        return tuple(outs)

    def pipeline_batch(self, frames, out=None, outputs=None, dtype=None):
        """pipeline() for n same-size frames in one launch.  frames: [n, H, W] tensor/array (or a list
        of planes).  outputs: indices into (g, h, e, magnitude, phase, edges, dark, bright) to
        produce (default all 8); returns / fills out [n, len(outputs), H, W] -- float32, or uint8 (a uint8 `out`, or dtype=uint8:
        8-bit maps as set_u8_gain says).  select_frame(i) then
        picks whose state the getters and steer() use (unless set_persist(False))."""
        sel = list(range(8)) if outputs is None else [int(k) for k in outputs]
        u8 = self._u8_dtype(dtype)
        block = _is_torch(frames) and frames.dim() == 3 and frames.dtype in (torch.float32, torch.uint8) and frames.is_cuda
        if block and out is None:
            out = torch.empty((frames.shape[0], len(sel)) + tuple(frames.shape[1:]), dtype=torch.uint8 if u8 else torch.float32, device=frames.device)
        if block and _is_torch(out) and out.dim() == 4 and out.is_cuda and out.dtype in (torch.float32, torch.uint8) \
                and out.shape[0] == frames.shape[0] and out.shape[1] == len(sel) and frames.stride(2) == 1 and out.stride(3) == 1:
            # one [n, H, W] block in, one [n, K, H, W] block out: the plane descriptors are filled in arithmetically
            # (two numpy arrays laid out like `struct cvs_plane`), not one Python object per plane
            n, rows, cols = (int(v) for v in frames.shape)
            self._like = frames[0]
            self._bind_stream(frames, out)
            imgs = np.zeros(n, _PLANE_DTYPE)
            esz = 1 if frames.dtype == torch.uint8 else 4   # 8-bit frames are read as bytes by the kernel (CVS_DEPTH_U8)
            imgs["data"] = frames.data_ptr() + np.arange(n, dtype=np.uint64) * np.uint64(frames.stride(0) * esz)
            imgs["rows"], imgs["cols"], imgs["step"] = rows, cols, frames.stride(1) * esz
            imgs["mem"] = L.MEM_DEVICE | (L.DEPTH_U8 if esz == 1 else 0)
            outs = np.zeros((n, 8), _PLANE_DTYPE)  # data == NULL means "not requested"
            osz = 1 if out.dtype == torch.uint8 else 4   # 8-bit outputs: steps in bytes (CVS_DEPTH_U8)
            frame_off = np.arange(n, dtype=np.uint64) * np.uint64(out.stride(0) * osz)
            for j, k in enumerate(sel):
                outs["data"][:, k] = out.data_ptr() + frame_off + np.uint64(j * out.stride(1) * osz)
                outs["rows"][:, k], outs["cols"][:, k], outs["step"][:, k] = rows, cols, out.stride(2) * osz
                outs["mem"][:, k] = L.MEM_DEVICE | (L.DEPTH_U8 if osz == 1 else 0)
            self._check(lib().cvs_pipeline_batch(self._h, imgs.ctypes.data_as(L._PP), n, outs.ctypes.data_as(L._PP)), "cvs_pipeline_batch")
            self._batch_keepalive = (frames, out)
            return out
        planes = [_as_input(f) for f in frames]
        n = len(planes)
        self._like = planes[0]
        shape = tuple(planes[0].shape)
        if out is None:
            if _is_torch(planes[0]):
                out = torch.empty((n, len(sel)) + shape, dtype=torch.uint8 if u8 else torch.float32, device=planes[0].device)
            else:
                out = np.empty((n, len(sel)) + shape, np.uint8 if u8 else np.float32)
        self._bind_stream(planes[0], out[0][0])
        imgs = _planes(planes)
        outs = (Plane * (n * 8))()  # zero-initialised: data == NULL means "not requested"
        for i in range(n):
            for j, k in enumerate(sel):
                outs[i * 8 + k] = _plane(out[i][j])
        self._check(lib().cvs_pipeline_batch(self._h, imgs, n, outs), "cvs_pipeline_batch")
        self._batch_keepalive = (planes, out)
        return out

    # -- contour thinning (extension beyond the reference): cvs_nonmax / cvs_hysteresis --
    @staticmethod
    def _plane_list(maps, most, what):
        single = (_is_torch(maps) or isinstance(maps, np.ndarray)) and maps.ndim == 2
        ms = [maps] if single else list(maps)
        if not 1 <= len(ms) <= most:
            raise ValueError("%s: one plane or a sequence of 1..%d planes" % (what, most))
        return single, ms

    def nonmax(self, maps, theta=None, out=None):
        """Thin maps (one plane or a sequence of up to 3, e.g. edges / dark / bright) to their local maxima across the orientation
        theta (cvs_nonmax): kept pixels keep their value, all others are 0.  theta=None: the object's dominant orientation (of the
        frame select_frame chose).  Returns the same shape as `maps`: one plane, or a tuple."""
        self._caller_check("cvs_nonmax")
        single, ms = self._plane_list(maps, 3, "nonmax")
        outs = [self._new_like(m) for m in ms] if out is None else ([out] if single else list(out))
        if len(outs) != len(ms):
            raise ValueError("out: one plane per map")
        self._bind_stream(*ms, *outs, *([] if theta is None else [theta]))
        n = len(ms)
        pin, pout = _planes(ms), _planes(outs)
        pt = None if theta is None else C.byref(_plane(theta))
        self._check(lib().cvs_nonmax(self._h, pt, n, pin, pout), "cvs_nonmax")
        return outs[0] if single else tuple(outs)

    def hysteresis(self, maps, low, high, dtype=torch.uint8 if torch is not None else np.uint8, out=None, return_passes=False):
        """8-connected hysteresis (cvs_hysteresis): 255 where a pixel is > high, or in (low, high] and connected through such pixels to
        one > high; 0 elsewhere.  maps: one plane or a sequence; dtype uint8 (bytes) or float32 (0.0 / 255.0).  Returns the same shape
        as `maps`, and with return_passes=True also the number of propagation passes run."""
        self._caller_check("cvs_hysteresis")
        single, ms = self._plane_list(maps, 1 << 30, "hysteresis")
        u8 = self._u8_dtype(dtype)
        outs = self._mask_outs(ms, u8, out, single, "map")
        self._bind_stream(*ms, *outs)
        n = len(ms)
        pin, pout = _planes(ms), _planes(outs)
        passes = C.c_int(0)
        self._check(lib().cvs_hysteresis(self._h, n, pin, float(low), float(high), pout, C.byref(passes)), "cvs_hysteresis")
        res = outs[0] if single else tuple(outs)
        return (res, passes.value) if return_passes else res

    # -- contour components (extension beyond the reference): cvs_label / cvs_component_stats / cvs_contour_prune / cvs_contour_points --
    COMPONENT_DTYPE = np.dtype([("area", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("first_x", "<i4"),
                                ("first_y", "<i4"), ("peak_x", "<i4"), ("peak_y", "<i4"), ("peak", "<f4")])

    @staticmethod
    def _new_typed_like(a, dtype_np):
        if _is_torch(a):
            return torch.empty(tuple(a.shape), dtype=getattr(torch, np.dtype(dtype_np).name), device=a.device)
        return np.empty(a.shape, dtype_np)

    def _mask_outs(self, ms, u8, out, single, what):
        """The outputs of hysteresis / prune / link: `out` as given, or a new plane like each input, bytes or f32."""
        if out is None:
            outs = [self._new_typed_like(m, np.uint8 if u8 else np.float32) for m in ms]
        else:
            outs = [out] if single else list(out)
        if len(outs) != len(ms):
            raise ValueError("out: one plane per %s" % what)
        return outs

    def label(self, mask, out=None):
        """8-connected components of a mask (cvs_label): float32 (foreground: > 0) or uint8 (non-zero).  Returns (labels, count): an
        int32 plane like `mask`, 0 for background and 1 .. count in raster order of each component's first pixel."""
        labels = self._new_typed_like(mask, np.int32) if out is None else out
        self._bind_stream(mask, labels)
        pm, pl = _plane(mask), _plane(labels)
        count = C.c_int(0)
        self._check(lib().cvs_label(self._h, C.byref(pm), C.byref(pl), C.byref(count)), "cvs_label")
        return labels, count.value

    def component_stats(self, labels, count, weight=None):
        """One record per label 1 .. count (cvs_component_stats): a numpy structured array with the fields of `cvs_component`
        (area, x0, y0, x1, y1, first_x, first_y, peak_x, peak_y, peak); weight: the float32 plane whose maximum is the peak."""
        table = np.zeros(int(count), self.COMPONENT_DTYPE)
        self._bind_stream(labels, *([] if weight is None else [weight]))
        pl = _plane(labels)
        pw = None if weight is None else C.byref(_plane(weight))
        self._check(lib().cvs_component_stats(self._h, C.byref(pl), int(count), pw, C.c_void_p(table.ctypes.data if count else None),
                                              L.MEM_HOST), "cvs_component_stats")
        return table

    def prune(self, masks, min_area, weight=None, min_peak=0.0, dtype=torch.uint8 if torch is not None else np.uint8, out=None,
              return_kept=False):
        """Drop the short and the faint contours (cvs_contour_prune): 255 on every 8-connected component of a mask with at least
        min_area pixels and -- with `weight` planes -- a largest weight >= min_peak; 0 elsewhere.  masks: one plane or a sequence, like
        hysteresis; dtype uint8 or float32.  With return_kept=True also the number of components kept (per plane)."""
        single, ms = self._plane_list(masks, 1 << 30, "prune")
        ws = None if weight is None else self._plane_list(weight, 1 << 30, "prune")[1]
        if ws is not None and len(ws) != len(ms):
            raise ValueError("weight: one plane per mask")
        u8 = self._u8_dtype(dtype)
        outs = self._mask_outs(ms, u8, out, single, "mask")
        self._bind_stream(*ms, *outs, *(ws or []))
        n = len(ms)
        pin, pout = _planes(ms), _planes(outs)
        pw = None if ws is None else _planes(ws)
        kept = (C.c_int * n)()
        self._check(lib().cvs_contour_prune(self._h, n, pin, pw, int(min_area), float(min_peak), pout, kept), "cvs_contour_prune")
        res = outs[0] if single else tuple(outs)
        if return_kept:
            return res, (kept[0] if single else list(kept))
        return res

    def contour_points(self, labels, group=False):
        """(x, y, label) of every labelled pixel in raster order (cvs_contour_points): an (N, 3) int32 tensor / array like `labels`.
        group=True: a stable sort by label on top, returned with the offsets -- pts[off[k - 1]:off[k]] are the pixels of contour k in
        raster order (off has max label + 1 entries)."""
        self._bind_stream(labels)
        pl = _plane(labels)
        n = C.c_int(0)
        rc = lib().cvs_contour_points(self._h, C.byref(pl), None, 0, L.MEM_HOST, C.byref(n))
        if not (rc == L.E_SIZE and n.value):   # (E_SIZE with a count: the sizing answer; without one: a plane of another size)
            self._check(rc, "cvs_contour_points")
        dev = _is_torch(labels) and labels.is_cuda
        if dev:
            pts = torch.empty((n.value, 3), dtype=torch.int32, device=labels.device)
        else:
            pts = np.empty((n.value, 3), np.int32)
        if n.value:
            ptr = C.c_void_p(pts.data_ptr() if dev else pts.ctypes.data)
            self._check(lib().cvs_contour_points(self._h, C.byref(pl), ptr, n.value, L.MEM_DEVICE if dev else L.MEM_HOST, C.byref(n)),
                        "cvs_contour_points")
        if _is_torch(labels) and not dev:
            pts = torch.from_numpy(pts)
        if not group:
            return pts
        if _is_torch(pts):
            order = torch.sort(pts[:, 2], stable=True).indices
            pts = pts[order]
            top = int(pts[-1, 2]) if len(pts) else 0
            off = torch.zeros(top + 1, dtype=torch.int64, device=pts.device)
            if len(pts):
                off[1:] = torch.cumsum(torch.bincount(pts[:, 2].long(), minlength=top + 1)[1:], 0)
        else:
            pts = pts[np.argsort(pts[:, 2], kind="stable")]
            top = int(pts[-1, 2]) if len(pts) else 0
            off = np.zeros(top + 1, np.int64)
            if len(pts):
                off[1:] = np.cumsum(np.bincount(pts[:, 2], minlength=top + 1)[1:])
        return pts, off

    def contour_chains(self, mask):
        """The linked contours of a mask as ordered chains of pixels, cut at junctions and free ends (cvs_contour_chains).  Returns
        (points, chains): an (N, 2) int32 array of (x, y) and an (M, 4) int32 array of (start, length, flags, 0) -- chain c is
        points[start:start + length], flags a sum of CHAIN_CLOSED, CHAIN_HEAD_JUNCTION, CHAIN_TAIL_JUNCTION.  Torch tensors on the
        mask's device for a device mask, numpy arrays for a numpy mask.  The order of chains and points depends on the mask alone
        (include/cvsteer_hip.h has the contract)."""
        self._bind_stream(mask)
        pm = _plane(mask)
        n, m = C.c_int(0), C.c_int(0)
        rc = lib().cvs_contour_chains(self._h, C.byref(pm), None, 0, None, 0, L.MEM_HOST, C.byref(n), C.byref(m))
        if not (rc == L.E_SIZE and (n.value or m.value)):   # (E_SIZE with counts: the sizing answer; without: a plane of another size)
            self._check(rc, "cvs_contour_chains")
        dev = _is_torch(mask) and mask.is_cuda
        if dev:
            pts = torch.empty((n.value, 2), dtype=torch.int32, device=mask.device)
            chains = torch.empty((m.value, 4), dtype=torch.int32, device=mask.device)
        else:
            pts, chains = np.empty((n.value, 2), np.int32), np.empty((m.value, 4), np.int32)
        if n.value:
            pp = C.c_void_p(pts.data_ptr() if dev else pts.ctypes.data)
            pc = C.c_void_p(chains.data_ptr() if dev else chains.ctypes.data)
            self._check(lib().cvs_contour_chains(self._h, C.byref(pm), pp, n.value, pc, m.value, L.MEM_DEVICE if dev else L.MEM_HOST,
                                                 C.byref(n), C.byref(m)), "cvs_contour_chains")
        if _is_torch(mask) and not dev:
            pts, chains = torch.from_numpy(pts), torch.from_numpy(chains)
        return pts, chains

    def chain_polylines(self, points, chains, eps, return_index=False):
        """Simplify every chain to a polyline (cvs_chain_polylines): Ramer-Douglas-Peucker with tolerance eps (pixels; inf keeps the
        end points only) on all chains at once.  points (N, 2) int32 and chains (M, 4) int32 as contour_chains returns them.  Returns
        (vertices (V, 2) int32, polylines (M, 4) int32 of (start, length, flags, 0)[, index (V,) int32: vertex k is points[index[k]]]).
        Torch CUDA tensors take the device path and give tensors on their device; numpy arrays take the host path (torch CPU tensors
        too, and come back as such).  Which points are kept depends on the inputs alone (include/cvsteer_hip.h has the contract)."""
        dev = _is_torch(points) and points.is_cuda
        if dev != (_is_torch(chains) and chains.is_cuda):
            raise ValueError("points and chains: both on the device or both on the host")
        back = _is_torch(points) and not dev
        if dev:
            points, chains = points.to(torch.int32).contiguous(), chains.to(torch.int32).contiguous()
        else:
            points = np.ascontiguousarray(points.numpy() if _is_torch(points) else points, np.int32)
            chains = np.ascontiguousarray(chains.numpy() if _is_torch(chains) else chains, np.int32)
        if points.ndim != 2 or points.shape[1] != 2 or chains.ndim != 2 or chains.shape[1] != 4:
            raise ValueError("points must be (N, 2) and chains (M, 4)")
        n, m = int(points.shape[0]), int(chains.shape[0])
        if dev:
            self._bind_stream(points)
            vtx = torch.empty((n, 2), dtype=torch.int32, device=points.device)
            idx = torch.empty((n,), dtype=torch.int32, device=points.device) if return_index else None
            tab = torch.empty((m, 4), dtype=torch.int32, device=points.device)
            ptr = lambda t: None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())
        else:
            vtx, idx, tab = np.empty((n, 2), np.int32), (np.empty((n,), np.int32) if return_index else None), np.empty((m, 4), np.int32)
            ptr = lambda t: None if t is None or t.size == 0 else C.c_void_p(t.ctypes.data)
        v = C.c_int(0)
        self._check(lib().cvs_chain_polylines(self._h, ptr(points), n, ptr(chains), m, float(eps), ptr(vtx), n, ptr(idx), ptr(tab),
                                              L.MEM_DEVICE if dev else L.MEM_HOST, C.byref(v)), "cvs_chain_polylines")
        vtx = vtx[:v.value]
        idx = None if idx is None else idx[:v.value]
        if back:
            vtx, tab, idx = torch.from_numpy(vtx), torch.from_numpy(tab), (None if idx is None else torch.from_numpy(idx))
        return (vtx, tab, idx) if return_index else (vtx, tab)

    def contour_polylines(self, mask, eps, return_index=False):
        """contour_chains(mask) followed by chain_polylines(..., eps): the linked contours of a mask as polylines.  With
        return_index=True the index refers to the points of contour_chains(mask)."""
        points, chains = self.contour_chains(mask)
        return self.chain_polylines(points, chains, eps, return_index=return_index)

    # -- contour edgels (extension beyond the reference): cvs_chain_refine / cvs_chain_measures --
    MEASURE_DTYPE = np.dtype([("axial", "<i4"), ("diagonal", "<i4"), ("other", "<i4"), ("peak_index", "<i4"), ("peak", "<f4"),
                              ("weakest", "<f4"), ("sum", "<f8"), ("length", "<f8")])

    @staticmethod
    def _chain_array(a, dev, dtype_np, width, what):
        """`a` as a contiguous array of `dtype_np` with `width` columns (0: one-dimensional): a CUDA tensor when dev, else numpy"""
        if a is None:
            return None
        if dev:
            if not (_is_torch(a) and a.is_cuda):
                raise ValueError("%s: on the device like points" % what)
            a = a.to(getattr(torch, np.dtype(dtype_np).name)).contiguous()
        else:
            if _is_torch(a) and a.is_cuda:
                raise ValueError("%s: on the host like points" % what)
            a = np.ascontiguousarray(a.numpy() if _is_torch(a) else a, dtype_np)
        if (a.ndim != 2 or a.shape[1] != width) if width else a.ndim != 1:
            raise ValueError("%s must be %s" % (what, "(N, %d)" % width if width else "(N,)"))
        return a

    @staticmethod
    def _is_out(a, dev, dtype_np, shape):
        """is `a` a contiguous array of that type and shape where the call writes: a CUDA tensor when dev, else a numpy array"""
        if dev:
            return _is_torch(a) and a.is_cuda and a.dtype == getattr(torch, np.dtype(dtype_np).name) and tuple(a.shape) == shape and a.is_contiguous()
        return isinstance(a, np.ndarray) and a.dtype == dtype_np and a.shape == shape and a.flags.c_contiguous

    @staticmethod
    def _array_ptr(a):
        if a is None or (a.numel() if _is_torch(a) else a.size) == 0:
            return None
        return C.c_void_p(a.data_ptr() if _is_torch(a) else a.ctypes.data)

    def chain_refine(self, points, map, theta=None, out=None):
        """Sub-pixel position and strength of every chain point (cvs_chain_refine).  points: (N, 2) int32 of (x, y) as contour_chains
        returns them; map: the UN-THINNED response the contours were found in (the edges / dark / bright output of pipeline, not the
        output of nonmax); theta=None: the object's dominant orientation (of the frame select_frame chose).  Returns (xy (N, 2) float32
        of (xs, ys), strength (N,) float32).  Torch CUDA points take the device path -- one launch, nothing read back, capturable -- and
        give tensors on their device; numpy points take the host path (torch CPU tensors too, and come back as such).  out: an
        (xy, strength) pair to write into instead.  include/cvsteer_hip.h has the contract."""
        if theta is None:
            self._caller_check("cvs_chain_refine")   # (the object's own orientation: G4 has one with extensions only)
        dev = _is_torch(points) and points.is_cuda
        back = _is_torch(points) and not dev
        points = self._chain_array(points, dev, np.int32, 2, "points")
        n = int(points.shape[0])
        if out is not None:
            xy, strength = out
            if not (self._is_out(xy, dev, np.float32, (n, 2)) and self._is_out(strength, dev, np.float32, (n,))):
                raise ValueError("out: contiguous float32 (N, 2) and (N,) arrays, where points are")
        elif dev:
            xy = torch.empty((n, 2), dtype=torch.float32, device=points.device)
            strength = torch.empty((n,), dtype=torch.float32, device=points.device)
        else:
            xy, strength = np.empty((n, 2), np.float32), np.empty((n,), np.float32)
        self._bind_stream(points, map, *([] if theta is None else [theta]))
        pm = _plane(map)
        pt = None if theta is None else C.byref(_plane(theta))
        self._check(lib().cvs_chain_refine(self._h, C.byref(pm), pt, self._array_ptr(points), n, self._array_ptr(xy), self._array_ptr(strength),
                                           L.MEM_DEVICE if dev else L.MEM_HOST), "cvs_chain_refine")
        if back and out is None:
            xy, strength = torch.from_numpy(xy), torch.from_numpy(strength)
        return xy, strength

    def _table_call(self, name, arrays, held, tables, args, out, out_text):
        """What chain_measures, polyline_segments, chain_turns and chain_joins share around their C call `name`.  arrays: (label, array,
        dtype, width) in the order they are converted, points first -- where the points are decides the path (Torch CUDA: the device
        path); held: (labels, of, text) -- the arrays that hold one entry per entry of array `of`, and the ValueError if one does not;
        tables: (record dtype, rows(count)) of every table the call writes, count[label] being the entries of an array; out: None, or
        the caller's own uint8 CUDA tensor (a sequence of them for several tables), else ValueError(out_text); args(ptr, count, tab):
        the C arguments between the handle and `mem`.  Returns `out` if given, else the list of tables as structured numpy arrays."""
        dev = _is_torch(arrays[0][1]) and arrays[0][1].is_cuda
        a = {label: self._chain_array(x, dev, dtype_np, width, label) for label, x, dtype_np, width in arrays}
        count = {label: int(x.shape[0]) for label, x in a.items() if x is not None}
        for labels, of, text in held:
            if any(a[l] is not None and a[l].shape[0] != count[of] for l in labels):
                raise ValueError(text)
        shapes = [(rows(count), dt.itemsize) for dt, rows in tables]
        if out is not None:
            tabs = [out] if len(tables) == 1 else list(out)
            if not (dev and len(tabs) == len(tables) and all(self._is_out(t, dev, np.uint8, sh) for t, sh in zip(tabs, shapes))):
                raise ValueError(out_text)
        elif dev:
            tabs = [torch.empty(sh, dtype=torch.uint8, device=a[arrays[0][0]].device) for sh in shapes]
        else:
            tabs = [np.zeros(sh[0], dt) for (dt, _), sh in zip(tables, shapes)]
        if dev:
            self._bind_stream(a[arrays[0][0]])
        ptr = {label: self._array_ptr(x) for label, x in a.items()}
        self._check(getattr(lib(), name)(self._h, *args(ptr, count, [self._array_ptr(t) for t in tabs]), L.MEM_DEVICE if dev else L.MEM_HOST),
                    name)
        if out is not None:
            return out
        return [t.cpu().numpy().view(dt).reshape(sh[0]) for t, (dt, _), sh in zip(tabs, tables, shapes)] if dev else tabs

    def chain_measures(self, points, chains, strength=None, xy=None, out=None):
        """One record per chain (cvs_chain_measures): a numpy structured array with the fields of `cvs_chain_measure` (axial, diagonal,
        other: steps by kind; peak_index, peak, weakest, sum of `strength`; length: the Euclidean length, of the sub-pixel `xy` when
        given, else of the integer points).  points (N, 2) int32 and chains (M, 4) int32 as contour_chains returns them, strength (N,)
        and xy (N, 2) float32 as chain_refine returns them.  Torch CUDA arrays take the device path: the table is written on the device
        and downloaded for the return value -- or, with out= an (M, 40) uint8 CUDA tensor, left there (nothing read back, capturable;
        out.cpu().numpy().view(MEASURE_DTYPE) reads it) and `out` is returned."""
        size = self.MEASURE_DTYPE.itemsize
        r = self._table_call(
            "cvs_chain_measures",
            [("points", points, np.int32, 2), ("chains", chains, np.int32, 4), ("strength", strength, np.float32, 0), ("xy", xy, np.float32, 2)],
            [(("strength", "xy"), "points", "strength and xy: one entry per point")], [(self.MEASURE_DTYPE, lambda c: c["chains"])],
            lambda p, c, t: (p["points"], c["points"], p["chains"], c["chains"], p["xy"], p["strength"], t[0]),
            out, "out: a contiguous (M, %d) uint8 CUDA tensor, with device arrays" % size)
        return r if out is not None else r[0]

    def contour_edgels(self, mask, map, theta=None):
        """contour_chains(mask), chain_refine on the un-thinned `map` the mask came from, chain_measures on both: the linked contours of
        a mask as sub-pixel edgels.  Returns (points, chains, xy, strength, measures)."""
        points, chains = self.contour_chains(mask)
        xy, strength = self.chain_refine(points, map, theta)
        return points, chains, xy, strength, self.chain_measures(points, chains, strength=strength, xy=xy)

    # -- contour segments (extension beyond the reference): cvs_polyline_segments --
    SEGMENT_DTYPE = np.dtype([("first", "<i4"), ("count", "<i4"), ("chain", "<i4"), ("flags", "<i4")] +
                             [(name, "<f8") for name in ("w", "sx", "sy", "sxx", "sxy", "syy", "cx", "cy", "ux", "uy", "t0", "t1", "rms", "dmax")])

    def polyline_segments(self, points, chains, polylines, index, xy=None, strength=None, out=None):
        """One record per polyline vertex (cvs_polyline_segments): a numpy structured array with the fields of `cvs_segment` -- record k is
        the total-least-squares line through the points of the span that starts at vertex k (first, count, chain, flags; the weighted
        moments w .. syy about the span's first pixel; the line (cx, cy) + t (ux, uy), t in [t0, t1]; rms and dmax, the RMS and largest
        distance of the points from it); count 0 where no span starts (the last vertex of an open polyline).  points (N, 2) int32 and
        chains (M, 4) int32 as contour_chains returns them, polylines (M, 4) and index (V,) int32 as chain_polylines(return_index=True)
        does, xy (N, 2) and strength (N,) float32 as chain_refine does: xy=None fits the integer points, strength=None weighs every point 1.
        Torch CUDA arrays take the device path: the table is written on the device and downloaded for the return value -- or, with out= a
        (V, 128) uint8 CUDA tensor, left there (two launches, nothing read back, capturable; out.cpu().numpy().view(SEGMENT_DTYPE) reads
        it) and `out` is returned.  numpy arrays and torch CPU tensors take the host path.  include/cvsteer_hip.h has the contract."""
        size = self.SEGMENT_DTYPE.itemsize
        r = self._table_call(
            "cvs_polyline_segments",
            [("points", points, np.int32, 2), ("chains", chains, np.int32, 4), ("polylines", polylines, np.int32, 4),
             ("index", index, np.int32, 0), ("xy", xy, np.float32, 2), ("strength", strength, np.float32, 0)],
            [(("polylines",), "chains", "polylines: one entry per chain"), (("strength", "xy"), "points", "strength and xy: one entry per point")],
            [(self.SEGMENT_DTYPE, lambda c: c["index"])],
            lambda p, c, t: (p["points"], c["points"], p["chains"], p["polylines"], c["chains"], p["index"], c["index"], p["xy"], p["strength"],
                             t[0]),
            out, "out: a contiguous (V, %d) uint8 CUDA tensor, with device arrays" % size)
        return r if out is not None else r[0]

    def contour_segments(self, mask, map, eps, theta=None, weighted=False, min_points=2):
        """The straight segments of the linked contours of a mask, to sub-pixel accuracy: contour_chains(mask) ->
        chain_polylines(eps, return_index=True) -> chain_refine on the un-thinned `map` the mask came from -> polyline_segments on the
        refined positions (weighted=True: weighted by the refined strengths).  Returns (segments, lines): the records with
        count >= min_points that are not SEG_DEGENERATE, and their (N, 4) float64 end points (cx + t0 ux, cy + t0 uy, cx + t1 ux,
        cy + t1 uy)."""
        points, chains = self.contour_chains(mask)
        _, polylines, index = self.chain_polylines(points, chains, eps, return_index=True)
        xy, strength = self.chain_refine(points, map, theta)
        seg = self.polyline_segments(points, chains, polylines, index, xy=xy, strength=strength if weighted else None)
        seg = seg[(seg["count"] >= min_points) & ((seg["flags"] & L.SEG_DEGENERATE) == 0)]
        lines = np.stack([seg["cx"] + seg["t0"] * seg["ux"], seg["cy"] + seg["t0"] * seg["uy"],
                          seg["cx"] + seg["t1"] * seg["ux"], seg["cy"] + seg["t1"] * seg["uy"]], axis=1).reshape(-1, 4)
        return seg, lines

    # -- contour turns (extension beyond the reference): cvs_chain_turns --
    TURN_DTYPE = np.dtype([("chain", "<i4"), ("flags", "<i4"), ("nb", "<i4"), ("nf", "<i4"), ("sin", "<f4"), ("cos", "<f4"), ("lb", "<f4"),
                           ("lf", "<f4")])
    TURN_SUMMARY_DTYPE = np.dtype([("corners", "<i4"), ("eligible", "<i4"), ("sharpest", "<i4"), ("min_cos", "<f4")])

    def chain_turns(self, points, chains, xy=None, radius=5, min_arm=None, nms=None, max_cos=0.70710678, summary=False, out=None):
        """One record per chain point (cvs_chain_turns): a numpy structured array with the fields of `cvs_chain_turn` -- record i holds the
        turn of the contour at point i between the direction towards it from the centroid of the `radius` points before it and the
        direction from it to the centroid of the `radius` points after it (chain, flags, the arm sizes nb and nf, sin and cos of the turn,
        the arm lengths lb and lf); flags & TURN_CORNER marks the corners: eligible points (both arms of min_arm points or more) with
        cos <= max_cos that are the sharpest within `nms` points either way, the first of a plateau.  min_arm and nms default to radius,
        max_cos to cos 45 deg.  points (N, 2) int32 and chains (M, 4) int32 as contour_chains returns them, xy (N, 2) float32 as
        chain_refine does: xy=None takes the integer points.  summary=True returns (turns, summary), the second a structured array with
        the fields of `cvs_turn_summary`, one per chain.  Torch CUDA arrays take the device path: the tables are written on the device
        and downloaded for the return value -- or, with out= an (N, 32) uint8 CUDA tensor (summary=True: a pair with an (M, 16) one), left
        there (two or three launches, nothing read back, capturable; out.cpu().numpy().view(TURN_DTYPE) reads it) and `out` is returned.
        numpy arrays and torch CPU tensors take the host path.  include/cvsteer_hip.h has the contract."""
        size, ssize = self.TURN_DTYPE.itemsize, self.TURN_SUMMARY_DTYPE.itemsize
        cfg = lambda: L.TurnCfg(int(radius), int(radius if min_arm is None else min_arm), int(radius if nms is None else nms), float(max_cos))
        r = self._table_call(
            "cvs_chain_turns", [("points", points, np.int32, 2), ("chains", chains, np.int32, 4), ("xy", xy, np.float32, 2)],
            [(("xy",), "points", "xy: one entry per point")],
            [(self.TURN_DTYPE, lambda c: c["points"])] + ([(self.TURN_SUMMARY_DTYPE, lambda c: c["chains"])] if summary else []),
            lambda p, c, t: (p["points"], c["points"], p["chains"], c["chains"], p["xy"], C.byref(cfg()), t[0], t[1] if summary else None),
            out, "out: a contiguous (N, %d) uint8 CUDA tensor%s, with device arrays" % (size, " and an (M, %d) one" % ssize if summary else ""))
        return r if out is not None else tuple(r) if summary else r[0]

    def contour_corners(self, mask, map, theta=None, **cfg):
        """The corners of the linked contours of a mask: contour_chains(mask) -> chain_refine on the un-thinned `map` the mask came from ->
        chain_turns on the refined positions (**cfg: its radius, min_arm, nms and max_cos).  Returns (corner_xy, corner_index, turns,
        chains): the (K, 2) float32 sub-pixel positions of the corners, their (K,) positions in the point list, the record of every
        point and the chain table."""
        points, chains = self.contour_chains(mask)
        xy, _ = self.chain_refine(points, map, theta)
        turns = self.chain_turns(points, chains, xy=xy, **cfg)
        index = np.nonzero(turns["flags"] & L.TURN_CORNER)[0]
        host_xy = xy.cpu().numpy() if _is_torch(xy) else np.asarray(xy)
        return host_xy[index], index, turns, chains

    # -- contour joins (extension beyond the reference): cvs_chain_joins --
    JOIN_DTYPE = np.dtype([("node", "<i4"), ("degree", "<i4"), ("next", "<i4"), ("partner", "<i4"), ("flags", "<i4"), ("n", "<i4"), ("cos", "<f4"),
                           ("sin", "<f4")])

    def chain_joins(self, points, chains, xy=None, radius=8, min_arm=None, min_cos=-1.0, out=None):
        """Two records per chain (cvs_chain_joins): a numpy structured array with the fields of `cvs_chain_join` -- record 2c is the head of
        chain c, record 2c + 1 its tail.  node, degree and next say which chain ends share the end's pixel (the smallest end number there,
        how many there are, the next one in the ring); partner is the end there that continues this one most nearly straight, judged on
        arms of up to `radius` points, cos and sin the turn from this end into it; flags & JOIN_MUTUAL marks the joins both ends agree on
        with cos >= min_cos.  An end whose arm has fewer than min_arm points (default min(3, radius)) joins nothing.  points (N, 2) int32
        and chains (M, 4) int32 as contour_chains or contour_chains_batch return them (ends of different planes never meet), xy (N, 2)
        float32 as chain_refine does: xy=None takes the integer points.  Torch CUDA arrays take the device path: the table is written on
        the device and downloaded for the return value -- or, with out= a (2M, 32) uint8 CUDA tensor, left there (three launches, nothing
        read back, capturable once the handle's scratch has its size; out.cpu().numpy().view(JOIN_DTYPE) reads it) and `out` is returned.
        numpy arrays and torch CPU tensors take the host path.  include/cvsteer_hip.h has the contract."""
        size = self.JOIN_DTYPE.itemsize
        cfg = lambda: L.JoinCfg(int(radius), int(min(3, radius) if min_arm is None else min_arm), float(min_cos), 0)
        r = self._table_call(
            "cvs_chain_joins", [("points", points, np.int32, 2), ("chains", chains, np.int32, 4), ("xy", xy, np.float32, 2)],
            [(("xy",), "points", "xy: one entry per point")], [(self.JOIN_DTYPE, lambda c: 2 * c["chains"])],
            lambda p, c, t: (p["points"], c["points"], p["chains"], c["chains"], p["xy"], C.byref(cfg()), t[0]),
            out, "out: a contiguous (2 M, %d) uint8 CUDA tensor, with device arrays" % size)
        return r if out is not None else r[0]

    def contour_joins(self, mask, map, theta=None, **cfg):
        """The joins of the linked contours of a mask: contour_chains(mask) -> chain_refine on the un-thinned `map` the mask came from ->
        chain_joins on the refined positions (**cfg: its radius, min_arm and min_cos).  Returns (joins, points, chains, xy)."""
        points, chains = self.contour_chains(mask)
        xy, _ = self.chain_refine(points, map, theta)
        return self.chain_joins(points, chains, xy=xy, **cfg), points, chains, xy

    # -- contour paths (extension beyond the reference): cvs_chain_paths --
    PATH_MEMBER_DTYPE = np.dtype([("chain", "<i4"), ("flags", "<i4"), ("path", "<i4"), ("start", "<i4")])
    PATH_INFO_DTYPE = np.dtype([("first_member", "<i4"), ("n_members", "<i4"), ("first_end", "<i4"), ("last_end", "<i4")])

    def chain_paths(self, points, chains, joins, xy=None, return_index=False, out=None):
        """Stitch the chains into paths over their MUTUAL joins (cvs_chain_paths).  points (N, 2) int32 and chains (M, 4) int32 as
        contour_chains or contour_chains_batch return them, joins as chain_joins returns it (the structured array) or as its out= tensor
        ((2M, 32) uint8), xy (N, 2) float32 as chain_refine does.  Returns (path_points, paths, members, info[, path_xy][, index]) trimmed
        to the counts: path_points (P, 2) int32 and paths (K, 4) int32 are again a (points, chains) pair -- path p is
        path_points[start:start + length], flags CHAIN_CLOSED for a cycle -- that every chain call takes as it is; members (structured,
        PATH_MEMBER_DTYPE: chain, flags & MEMBER_REVERSED, path, start) lists the chains of every path in walk order, info (structured,
        PATH_INFO_DTYPE) says which members a path has and through which ends it starts and leaves; path_xy (with xy) holds the refined
        position and index (return_index=True) the position in `points` of every path point.  Torch CUDA arrays take the device path:
        the launches read nothing back, and the eight bytes of the counts are read here, afterwards, to trim; path_points, paths, path_xy
        and index stay tensors on the device, members and info are downloaded.  With out= a tuple of full-size CUDA tensors
        (path_points (N, 2) int32, paths (M, 4) int32, members (M, 16) uint8, info (M, 16) uint8[, path_xy (N, 2) float32][, index (N,)
        int32], counts (2,) int32) nothing is read back at all (capturable once the handle's scratch has its size): `out` is returned
        untrimmed, counts says how much of each tensor holds a result.  numpy arrays and torch CPU tensors take the host path.
        include/cvsteer_hip.h has the contract."""
        dev = _is_torch(points) and points.is_cuda
        back = _is_torch(points) and not dev
        points = self._chain_array(points, dev, np.int32, 2, "points")
        chains = self._chain_array(chains, dev, np.int32, 4, "chains")
        xy = self._chain_array(xy, dev, np.float32, 2, "xy")
        n, m = int(points.shape[0]), int(chains.shape[0])
        if isinstance(joins, np.ndarray) and joins.dtype.names:
            joins = np.ascontiguousarray(joins).view(np.uint8).reshape(-1, self.JOIN_DTYPE.itemsize)
            if dev:
                joins = torch.from_numpy(joins).to(points.device)
        joins = self._chain_array(joins, dev, np.uint8, self.JOIN_DTYPE.itemsize, "joins")
        if joins.shape[0] != 2 * m:
            raise ValueError("joins: two records per chain")
        if xy is not None and xy.shape[0] != n:
            raise ValueError("xy: one entry per point")
        shapes = [(np.int32, (n, 2)), (np.int32, (m, 4)), (np.uint8, (m, 16)), (np.uint8, (m, 16))]
        shapes += [(np.float32, (n, 2))] if xy is not None else []
        shapes += [(np.int32, (n,))] if return_index else []
        shapes += [(np.int32, (2,))]
        if out is not None:
            bufs = list(out)
            if not (dev and len(bufs) == len(shapes) and all(self._is_out(b, dev, dt, sh) for b, (dt, sh) in zip(bufs, shapes))):
                raise ValueError("out: contiguous CUDA tensors (path_points (N, 2) int32, paths (M, 4) int32, members (M, 16) uint8, info "
                                 "(M, 16) uint8[, path_xy (N, 2) float32][, index (N,) int32], counts (2,) int32), with device arrays")
        elif dev:
            bufs = [torch.empty(sh, dtype=getattr(torch, np.dtype(dt).name), device=points.device) for dt, sh in shapes]
        else:
            bufs = [np.zeros(sh, dt) for dt, sh in shapes]
        if dev:
            self._bind_stream(points)
        it = iter(bufs)
        path_points, paths, members, info = next(it), next(it), next(it), next(it)
        path_xy = next(it) if xy is not None else None
        index = next(it) if return_index else None
        counts = next(it)
        p = self._array_ptr
        self._check(lib().cvs_chain_paths(self._h, p(points), n, p(chains), m, p(joins), p(xy), p(path_points), p(paths), p(info), p(members),
                                          p(index), p(path_xy), p(counts), L.MEM_DEVICE if dev else L.MEM_HOST), "cvs_chain_paths")
        if out is not None:
            return out
        k, q = (int(v) for v in (counts.cpu() if dev else counts).tolist())   # (device path: the one read-back, after the call)
        q = min(q, n)
        host = (lambda t: t.cpu().numpy()) if dev else (lambda t: t)
        info = host(info[:k]).view(self.PATH_INFO_DTYPE).reshape(-1)
        n_members = int(info["n_members"].sum())                              # (every valid chain is one member)
        r = [path_points[:q], paths[:k], host(members[:n_members]).view(self.PATH_MEMBER_DTYPE).reshape(-1), info]
        r += [path_xy[:q]] if xy is not None else []
        r += [index[:q]] if return_index else []
        if back:
            r = [torch.from_numpy(np.ascontiguousarray(t)) if i not in (2, 3) else t for i, t in enumerate(r)]
        return tuple(r)

    def contour_paths(self, mask, map, theta=None, **cfg):
        """The whole contours of a mask: contour_chains(mask) -> chain_refine on the un-thinned `map` the mask came from -> chain_joins on
        the refined positions (**cfg: its radius, min_arm and min_cos) -> chain_paths.  Returns (path_points, paths, members, info,
        path_xy): what chain_paths returns with xy."""
        points, chains = self.contour_chains(mask)
        xy, _ = self.chain_refine(points, map, theta)
        dev = _is_torch(points) and points.is_cuda
        if dev:
            table = torch.empty((2 * int(chains.shape[0]), self.JOIN_DTYPE.itemsize), dtype=torch.uint8, device=points.device)
            joins = self.chain_joins(points, chains, xy=xy, out=table, **cfg)   # (stays on the device)
        else:
            joins = self.chain_joins(points, chains, xy=xy, **cfg)
        return self.chain_paths(points, chains, joins, xy=xy)

    # -- contour bridges (extension beyond the reference): cvs_chain_bridges --
    BRIDGE_DTYPE = BRIDGE_DTYPE

    def chain_bridges(self, points, chains, xy=None, radius=8, min_arm=3, max_gap=8, min_cos=0.8, emit=True, capacity=None, out=None):
        """Bridge the gaps between free chain ends that face each other (cvs_chain_bridges).  points (N, 2) int32 and chains (M, 4) int32
        as contour_chains, contour_chains_batch or chain_paths return them, xy (N, 2) float32 as chain_refine does: xy=None takes the
        integer points.  Two free ends are paired when their pixels are 2 .. max_gap apart (Chebyshev), each points at the other within
        the cone min_cos -- judged on arms of up to `radius` points, at least min_arm -- and each is the other's nearest such end.
        Returns (bridges, out_points, out_chains, out_xy): bridges a numpy structured array (BRIDGE_DTYPE: partner, flags & BRIDGE_*, n,
        steps, bridge, start, cos, cos_partner), two records per chain; out_points (N + B, 2) int32 and out_chains (M + K, 4) int32 the
        inputs with every bridge appended as a chain of its own (a digital line from the one end pixel to the other, flags
        CHAIN_HEAD_JUNCTION | CHAIN_TAIL_JUNCTION) and the junction bit of every bridged end set: again a (points, chains) pair, on
        which chain_joins and chain_paths stitch through the bridges; out_xy (N + B, 2) float32 with xy, else None.  emit=False: the
        table alone, (bridges, None, None, None).  Torch CUDA arrays take the device path and give tensors on their device (bridges is
        downloaded).  capacity=None calls twice: once for the table and the counts, whose twelve bytes are then read back -- the ONE
        read-back -- and once more with arrays of exactly that size.  capacity=(points, chains) calls once with arrays of that size and
        returns what fitted of the bridges, a prefix.  out= a tuple of the caller's own CUDA tensors (bridges (2M, 32) uint8, out_points
        (P, 2) int32, out_chains (K, 4) int32[, out_xy (P, 2) float32 with xy], counts (3,) int32), P >= N and K >= M the capacities:
        one call, nothing read back at all (capturable once the handle's scratch has its size); `out` is returned, counts = (bridges,
        chains, points) in full whatever fitted.  numpy arrays and torch CPU tensors take the host path.  include/cvsteer_hip.h has the
        contract."""
        dev = _is_torch(points) and points.is_cuda
        back = _is_torch(points) and not dev
        points = self._chain_array(points, dev, np.int32, 2, "points")
        chains = self._chain_array(chains, dev, np.int32, 4, "chains")
        xy = self._chain_array(xy, dev, np.float32, 2, "xy")
        n, m = int(points.shape[0]), int(chains.shape[0])
        if xy is not None and xy.shape[0] != n:
            raise ValueError("xy: one entry per point")
        cfg = L.BridgeCfg(int(radius), int(min_arm), int(max_gap), float(min_cos))
        size = BRIDGE_DTYPE.itemsize
        p = self._array_ptr
        if dev:
            self._bind_stream(points)
            new = lambda shape, dt: torch.empty(shape, dtype=getattr(torch, np.dtype(dt).name), device=points.device)
        else:
            new = lambda shape, dt: np.zeros(shape, dt)

        def call(table, o_pts, cap_p, o_chn, cap_c, o_xy, counts):
            self._check(lib().cvs_chain_bridges(self._h, p(points), n, p(chains), m, p(xy), C.byref(cfg), p(table), p(o_pts), cap_p, p(o_chn), cap_c,
                                                p(o_xy), p(counts), L.MEM_DEVICE if dev else L.MEM_HOST), "cvs_chain_bridges")

        if out is not None:
            bufs = list(out)
            ok = dev and len(bufs) == (5 if xy is not None else 4) and all(_is_torch(b) and b.is_cuda and b.ndim >= 1 for b in bufs)
            if ok:
                cap_p, cap_c = int(bufs[1].shape[0]), int(bufs[2].shape[0])
                shapes = [(np.uint8, (2 * m, size)), (np.int32, (cap_p, 2)), (np.int32, (cap_c, 4))]
                shapes += [(np.float32, (cap_p, 2))] if xy is not None else []
                shapes += [(np.int32, (3,))]
                ok = cap_p >= max(n, 1) and cap_c >= max(m, 1) and all(self._is_out(b, dev, dt, sh) for b, (dt, sh) in zip(bufs, shapes))
            if not ok:
                raise ValueError("out: contiguous CUDA tensors (bridges (2 M, %d) uint8, out_points (P, 2) int32, out_chains (K, 4) int32[, out_xy "
                                 "(P, 2) float32], counts (3,) int32) with P >= N and K >= M, with device arrays" % size)
            call(bufs[0], bufs[1], cap_p, bufs[2], cap_c, bufs[3] if xy is not None else None, bufs[-1])
            return out
        table, counts = new((2 * m, size), np.uint8), new((3,), np.int32)
        records = lambda: (table.cpu().numpy() if dev else table).view(BRIDGE_DTYPE).reshape(-1)
        if not emit:
            call(table, None, 0, None, 0, None, counts)
            return records(), None, None, None
        if capacity is None:
            call(table, None, 0, None, 0, None, counts)
            _, cap_c, cap_p = (int(v) for v in (counts.cpu() if dev else counts).tolist())   # (device path: the one read-back)
            if cap_p < n:
                raise ValueError("more than 2^31 - 1 output points")
        else:
            cap_p, cap_c = (int(v) for v in capacity)
            if cap_p < n or cap_c < m:
                raise ValueError("capacity: (points, chains), at least the inputs")
        o_pts, o_chn = new((max(cap_p, 1), 2), np.int32), new((max(cap_c, 1), 4), np.int32)
        o_xy = None if xy is None else new((max(cap_p, 1), 2), np.float32)
        call(table, o_pts, cap_p, o_chn, cap_c, o_xy, counts)
        rec = records()
        if capacity is None:
            k, q = cap_c, cap_p
        else:                                                                                # what fitted: a prefix of the bridges
            b = rec[(rec["bridge"] >= 0) & (np.arange(len(rec)) < rec["partner"])]
            last = b["start"].astype(np.int64) + b["steps"]
            fits = (m + b["bridge"].astype(np.int64) < cap_c) & (b["start"] >= 0) & (last < cap_p)
            k = m + int(fits.sum())
            q = int(last[fits].max()) + 1 if fits.any() else n
        r = [o_pts[:q], o_chn[:k], None if o_xy is None else o_xy[:q]]
        if back:
            r = [None if t is None else torch.from_numpy(np.ascontiguousarray(t)) for t in r]
        return (rec,) + tuple(r)

    def contour_bridges(self, mask, map=None, theta=None, radius=8, min_arm=3, join_min_cos=-1.0, max_gap=8, min_cos=0.8):
        """The whole contours of a mask with their gaps bridged: contour_chains(mask) [-> chain_refine on the un-thinned `map` the mask
        came from, when given] -> chain_joins -> chain_paths -> chain_bridges on the paths -> chain_joins -> chain_paths.  radius and
        min_arm are those of both chain_joins and of chain_bridges, join_min_cos the min_cos of the joins, max_gap and min_cos those of
        the bridges.  The second chain_joins takes min(min_arm, 2), so that the shortest bridge -- three points, an arm of two -- is
        eligible.  Returns what the last chain_paths returns: (path_points, paths, members, info[, path_xy with map]); `members` names
        chains of the bridged table (the first pass's paths, then the bridges)."""
        points, chains = self.contour_chains(mask)
        xy = None if map is None else self.chain_refine(points, map, theta)[0]
        def stitch(points, chains, xy, arm):
            if _is_torch(points) and points.is_cuda:
                table = torch.empty((2 * int(chains.shape[0]), self.JOIN_DTYPE.itemsize), dtype=torch.uint8, device=points.device)
                joins = self.chain_joins(points, chains, xy=xy, radius=radius, min_arm=arm, min_cos=join_min_cos, out=table)   # (stays there)
            else:
                joins = self.chain_joins(points, chains, xy=xy, radius=radius, min_arm=arm, min_cos=join_min_cos)
            return self.chain_paths(points, chains, joins, xy=xy)

        r = stitch(points, chains, xy, int(min_arm))
        _, points, chains, xy = self.chain_bridges(r[0], r[1], xy=None if xy is None else r[4], radius=radius, min_arm=min_arm, max_gap=max_gap,
                                                   min_cos=min_cos)
        return stitch(points, chains, xy, min(int(min_arm), 2))

    def contours(self, image, low, high, min_area=0, min_peak=0.0):
        """Thin, linked contours of one image: pipeline(image) -> nonmax(edges, dark, bright) on the object's own theta ->
        hysteresis(low, high).  Returns three uint8 masks (edges, dark lines, bright lines).  min_area > 0 or min_peak > 0: the
        masks are pruned on top -- components of fewer pixels, or whose strongest thinned response is below min_peak, are dropped."""
        maps = self.pipeline(image)
        thin = self.nonmax(maps[5:8])
        masks = self.hysteresis(thin, low, high)
        if min_area == 0 and min_peak == 0.0:
            return masks
        return self.prune(masks, min_area, weight=thin, min_peak=min_peak)

    # -- the contour chain on the batch axis (extension): cvs_link / cvs_nonmax_batch / cvs_contours_batch --
    @staticmethod
    def _block_planes(t, lead):
        """cvs_plane descriptors of the planes of a CUDA tensor whose last two axes are (H, W), filled in arithmetically: a numpy array
        laid out like `struct cvs_plane`, one entry per index of the `lead` leading axes in C order"""
        esz = t.element_size()
        off = np.zeros((), np.int64)
        for ax in range(lead):
            shape = [1] * lead
            shape[ax] = t.shape[ax]
            off = off + (np.arange(t.shape[ax], dtype=np.int64) * (t.stride(ax) * esz)).reshape(shape)
        planes = np.zeros(int(np.prod(t.shape[:lead])), _PLANE_DTYPE)
        planes["data"] = (t.data_ptr() + np.broadcast_to(off, tuple(t.shape[:lead])).reshape(-1)).astype(np.uint64)
        planes["rows"], planes["cols"] = int(t.shape[-2]), int(t.shape[-1])
        planes["step"] = (t.stride(-2) if t.shape[-2] > 1 else t.shape[-1]) * esz
        planes["mem"] = L.MEM_DEVICE | (L.DEPTH_U8 if t.dtype == torch.uint8 else 0)
        return planes

    @staticmethod
    def _is_block(a, ndim, dtypes):
        return _is_torch(a) and a.is_cuda and a.dim() == ndim and a.dtype in dtypes and (a.shape[-1] <= 1 or a.stride(-1) == 1)

    def link(self, maps, low, high, min_area=0, min_peak=-np.inf, dtype=torch.uint8 if torch is not None else np.uint8, out=None,
             return_kept=False):
        """Hysteresis and prune in one labelling (cvs_link): 255 on every 8-connected component of { v > low } whose largest value is
        > high and >= min_peak and that has at least min_area pixels, 0 elsewhere -- byte for byte hysteresis(maps, low, high) followed by
        prune(that, min_area, weight=maps, min_peak=min_peak), without a read-back.  maps: one plane, a sequence of any length, or an
        [N, H, W] block (a CUDA tensor: the planes are then addressed by one stride); dtype uint8 or float32.  Returns the same shape as
        `maps`; with return_kept=True also the number of components kept per plane, as an int32 tensor on the device."""
        self._caller_check("cvs_link")
        u8 = self._u8_dtype(dtype)
        if self._is_block(maps, 3, (torch.float32,) if torch is not None else ()):
            if out is None:
                out = torch.empty(tuple(maps.shape), dtype=torch.uint8 if u8 else torch.float32, device=maps.device)
            if not self._is_block(out, 3, (torch.uint8, torch.float32)) or tuple(out.shape) != tuple(maps.shape):
                raise ValueError("out: a CUDA block shaped like maps")
            n, single, res = int(maps.shape[0]), False, out
            self._bind_stream(maps, out)
            pin = self._block_planes(maps, 1).ctypes.data_as(L._PP)
            pout = self._block_planes(out, 1).ctypes.data_as(L._PP)
            keep = (maps, out)
        else:
            single, ms = self._plane_list(maps, 1 << 30, "link")
            outs = self._mask_outs(ms, u8, out, single, "map")
            self._bind_stream(*ms, *outs)
            n = len(ms)
            pin, pout = _planes(ms), _planes(outs)
            res = outs[0] if single else tuple(outs)
            keep = (ms, outs)
        kept = None
        if return_kept:
            if torch is None:
                raise ValueError("return_kept: the counts stay on the device, which needs torch")
            kept = torch.empty(n, dtype=torch.int32, device="cuda:%d" % self.device)
            self._bind_stream(kept)
        self._check(lib().cvs_link(self._h, n, pin, float(low), float(high), int(min_area), float(min_peak), pout,
                                   C.c_void_p(kept.data_ptr()) if kept is not None else None), "cvs_link")
        self._link_keepalive = keep
        if return_kept:
            return res, (kept[0] if single else kept)
        return res

    def nonmax_batch(self, maps, theta=None, out=None):
        """nonmax() for F frames of K maps in one launch (cvs_nonmax_batch).  maps: an [F, K, H, W] block (K in 1..3), or a sequence of
        F sequences of K planes; theta: [F, H, W] (or F planes), None = the dominant orientation of frames 0 .. F-1 of the last
        pipeline_batch.  Returns / fills `out`, shaped like `maps`; every value is that of select_frame(i); nonmax(maps[i])."""
        self._caller_check("cvs_nonmax_batch")
        f32 = (torch.float32,) if torch is not None else ()
        if self._is_block(maps, 4, f32):
            if out is None:
                out = torch.empty(tuple(maps.shape), dtype=torch.float32, device=maps.device)
            if not self._is_block(out, 4, f32) or tuple(out.shape) != tuple(maps.shape):
                raise ValueError("out: a CUDA block shaped like maps")
            frames, k = int(maps.shape[0]), int(maps.shape[1])
            pin = self._block_planes(maps, 2).ctypes.data_as(L._PP)
            pout = self._block_planes(out, 2).ctypes.data_as(L._PP)
            flat_in, flat_out, res = [maps], [out], out
        else:
            rows_in = [list(fr) for fr in maps]
            frames, k = len(rows_in), len(rows_in[0]) if rows_in else 0
            if frames < 1 or not 1 <= k <= 3 or any(len(fr) != k for fr in rows_in):
                raise ValueError("nonmax_batch: F >= 1 frames of K maps each, K in 1..3")
            rows_out = [[self._new_like(m) for m in fr] for fr in rows_in] if out is None else [list(fr) for fr in out]
            if len(rows_out) != frames or any(len(fr) != k for fr in rows_out):
                raise ValueError("out: one plane per map")
            flat_in, flat_out = [m for fr in rows_in for m in fr], [o for fr in rows_out for o in fr]
            pin, pout = _planes(flat_in), _planes(flat_out)
            res = out if out is not None else [tuple(fr) for fr in rows_out]
        pt, ths = None, []
        if theta is not None:
            if self._is_block(theta, 3, f32):
                if int(theta.shape[0]) != frames:
                    raise ValueError("theta: one plane per frame")
                ths, pt = [theta], self._block_planes(theta, 1).ctypes.data_as(L._PP)
            else:
                ths = list(theta)
                if len(ths) != frames:
                    raise ValueError("theta: one plane per frame")
                pt = _planes(ths)
        self._bind_stream(*flat_in, *flat_out, *ths)
        self._check(lib().cvs_nonmax_batch(self._h, frames, k, pt, pin, pout), "cvs_nonmax_batch")
        self._nms_keepalive = (flat_in, flat_out, ths)
        return res

    def contours_batch(self, frames, low, high, min_area=0, min_peak=0.0):
        """contours() for n same-size frames (cvs_contours_batch): pipeline_batch -> nonmax_batch on every frame's own theta -> link.
        frames: [n, H, W] tensor / array (float32 or uint8) or a list of planes.  Returns [n, 3, H, W] uint8 -- (edges, dark, bright) per
        frame, each equal to contours(frame, ...) --, without a read-back for device frames; the object then holds the state of all n frames
        (select_frame).  As in contours(), min_area == 0 and min_peak == 0.0 means no peak test."""
        self._caller_check("cvs_contours_batch")
        if min_area == 0 and min_peak == 0.0:
            min_peak = -np.inf
        if self._is_block(frames, 3, (torch.float32, torch.uint8) if torch is not None else ()):
            planes, n = [frames], int(frames.shape[0])
            self._like = frames[0]
            out = torch.empty((n, 3) + tuple(frames.shape[1:]), dtype=torch.uint8, device=frames.device)
            pim = self._block_planes(frames, 1).ctypes.data_as(L._PP)
            pout = self._block_planes(out, 2).ctypes.data_as(L._PP)
        else:
            planes = [_as_input(f) for f in frames]
            n = len(planes)
            if n < 1:
                raise ValueError("contours_batch: at least one frame")
            self._like = planes[0]
            shape = (n, 3) + tuple(planes[0].shape)
            if _is_torch(planes[0]):
                out = torch.empty(shape, dtype=torch.uint8, device=planes[0].device)
            else:
                out = np.empty(shape, np.uint8)
            pim, pout = _planes(planes), _planes([out[i][k] for i in range(n) for k in range(3)])
        self._bind_stream(*planes, out)
        self._check(lib().cvs_contours_batch(self._h, pim, n, float(low), float(high), int(min_area), float(min_peak), pout),
                    "cvs_contours_batch")
        self._batch_keepalive = (planes, out)
        return out

    # -- contour chains and sub-pixel chain points on the batch axis (extension): cvs_contour_chains_batch / cvs_chain_refine_batch --
    def _plane_block(self, a, what):
        """the planes of `a` -- an [N, H, W] or [F, K, H, W] block (a CUDA tensor: descriptors filled in arithmetically), or a sequence of
        planes or of sequences of planes -- as (cvs_plane array pointer, number of planes, what to keep alive, leading shape)"""
        f32u8 = (torch.float32, torch.uint8) if torch is not None else ()
        for nd in (3, 4):
            if self._is_block(a, nd, f32u8):
                lead = tuple(int(v) for v in a.shape[:nd - 2])
                return self._block_planes(a, nd - 2).ctypes.data_as(L._PP), int(np.prod(lead)), [a], lead
        flat, lead = [], None
        for item in a:
            if (_is_torch(item) or isinstance(item, np.ndarray)) and item.ndim == 2:
                flat.append(item)
            else:
                row = list(item)
                if lead is not None and lead[1] != len(row):
                    raise ValueError("%s: the same number of planes in every frame" % what)
                lead = (0, len(row))
                flat.extend(row)
        if not flat:
            raise ValueError("%s: at least one plane" % what)
        lead = (len(flat),) if lead is None else (len(flat) // lead[1], lead[1])
        return _planes(flat), len(flat), flat, lead

    def contour_chains_batch(self, masks):
        """contour_chains for n masks in one launch sequence with one read-back (cvs_contour_chains_batch).  masks: an [N, H, W] or
        [F, K, H, W] block (uint8 or float32), or a sequence of planes, all on the device or all on the host.  Returns (points, chains,
        ranges): the concatenation over the planes z of contour_chains(masks[z]) -- points (P, 2) int32 of (x, y) inside their plane,
        chains (M, 4) int32 of (start, length, flags, plane) with start counting through all planes -- and ranges (n + 1, 2) int32:
        ranges[z] = (first chain, first point) of plane z, ranges[n] the totals.  The chains of plane z are chains[ranges[z, 0]:
        ranges[z + 1, 0]].  Tensors on the masks' device for CUDA masks, numpy arrays for numpy masks (torch CPU masks come back as
        torch CPU tensors).  chain_polylines and chain_measures take points and chains as they are; chain_refine_batch takes ranges."""
        pm, n, keep, _ = self._plane_block(masks, "contour_chains_batch")
        first = keep[0]
        self._bind_stream(*keep)
        dev = _is_torch(first) and first.is_cuda
        np_, nc = C.c_int(0), C.c_int(0)
        rc = lib().cvs_contour_chains_batch(self._h, n, pm, None, 0, None, 0, None, L.MEM_HOST, C.byref(np_), C.byref(nc))
        if not (rc == L.E_SIZE and (np_.value or nc.value)):   # (E_SIZE with counts: the sizing answer; without: a plane of another size)
            self._check(rc, "cvs_contour_chains_batch")
        if dev:
            pts = torch.empty((np_.value, 2), dtype=torch.int32, device=first.device)
            chains = torch.empty((nc.value, 4), dtype=torch.int32, device=first.device)
            ranges = torch.empty((n + 1, 2), dtype=torch.int32, device=first.device)
        else:
            pts, chains, ranges = np.empty((np_.value, 2), np.int32), np.empty((nc.value, 4), np.int32), np.empty((n + 1, 2), np.int32)
        self._check(lib().cvs_contour_chains_batch(self._h, n, pm, self._array_ptr(pts), np_.value, self._array_ptr(chains), nc.value,
                                                   self._array_ptr(ranges), L.MEM_DEVICE if dev else L.MEM_HOST, C.byref(np_), C.byref(nc)),
                    "cvs_contour_chains_batch")
        if _is_torch(first) and not dev:
            pts, chains, ranges = torch.from_numpy(pts), torch.from_numpy(chains), torch.from_numpy(ranges)
        return pts, chains, ranges

    def chain_refine_batch(self, points, ranges, maps, theta=None, out=None):
        """chain_refine for the point list of contour_chains_batch in one launch (cvs_chain_refine_batch).  points, ranges: as
        contour_chains_batch returns them for F * K planes; maps: the UN-THINNED responses the masks came from, an [F, K, H, W] block (K in
        1..3) or a sequence of F sequences of K planes; theta: [F, H, W] (or F planes), None = the dominant orientation of frames 0 .. F-1
        of the last pipeline_batch.  Returns (xy (P, 2) float32, strength (P,) float32), every value that of select_frame(z // K);
        chain_refine(points of plane z, maps[z // K][z % K]).  CUDA points take the device path -- nothing read back, capturable --; numpy
        points the host path (torch CPU tensors too, and come back as such).  out: an (xy, strength) pair to write into instead."""
        if theta is None:
            self._caller_check("cvs_chain_refine_batch")
        dev = _is_torch(points) and points.is_cuda
        back = _is_torch(points) and not dev
        points = self._chain_array(points, dev, np.int32, 2, "points")
        ranges = self._chain_array(ranges, dev, np.int32, 2, "ranges")
        pm, n, keep, lead = self._plane_block(maps, "chain_refine_batch")
        if len(lead) != 2 or not 1 <= lead[1] <= 3:
            raise ValueError("chain_refine_batch: maps are F frames of K planes each, K in 1..3")
        if int(ranges.shape[0]) != n + 1:
            raise ValueError("ranges: one row per plane and one for the totals")
        pt, ths = None, []
        if theta is not None:
            pt, nt, ths, _ = self._plane_block(theta, "theta")
            if nt != lead[0]:
                raise ValueError("theta: one plane per frame")
        npts = int(points.shape[0])
        if out is not None:
            xy, strength = out
            if not (self._is_out(xy, dev, np.float32, (npts, 2)) and self._is_out(strength, dev, np.float32, (npts,))):
                raise ValueError("out: contiguous float32 (N, 2) and (N,) arrays, where points are")
        elif dev:
            xy = torch.empty((npts, 2), dtype=torch.float32, device=points.device)
            strength = torch.empty((npts,), dtype=torch.float32, device=points.device)
        else:
            xy, strength = np.empty((npts, 2), np.float32), np.empty((npts,), np.float32)
        self._bind_stream(points, *keep, *ths)
        self._check(lib().cvs_chain_refine_batch(self._h, lead[0], lead[1], pm, pt, self._array_ptr(points), npts, self._array_ptr(ranges),
                                                 self._array_ptr(xy), self._array_ptr(strength), L.MEM_DEVICE if dev else L.MEM_HOST),
                    "cvs_chain_refine_batch")
        self._refine_keepalive = (points, ranges, keep, ths)
        if back and out is None:
            xy, strength = torch.from_numpy(xy), torch.from_numpy(strength)
        return xy, strength

    def contour_edgels_batch(self, frames, low, high, min_area=0, min_peak=0.0, eps=None):
        """The linked contours of n same-size frames as sub-pixel edgels, without a loop over frames or planes:
        pipeline_batch(outputs=[5, 6, 7]) -> nonmax_batch -> link -> contour_chains_batch -> chain_refine_batch -> chain_measures, and
        chain_polylines(..., return_index=True) when eps is given.  low, high, min_area, min_peak as in contours_batch.  Returns
        (points, chains, ranges, xy, strength, measures[, vertices, polylines, index]); plane z = 3 * frame + (0 edges, 1 dark lines,
        2 bright lines), and chains[:, 3] names it.  The object then holds the state of all n frames."""
        self._caller_check("contour_edgels_batch")
        if min_area == 0 and min_peak == 0.0:
            min_peak = -np.inf
        maps = self.pipeline_batch(frames, outputs=[5, 6, 7])
        thin = self.nonmax_batch(maps)
        if not (_is_torch(thin) or isinstance(thin, np.ndarray)):
            thin = [m for fr in thin for m in fr]
        else:
            thin = thin.reshape((-1,) + tuple(thin.shape[2:]))
        masks = self.link(thin, low, high, min_area=min_area, min_peak=min_peak)
        points, chains, ranges = self.contour_chains_batch(masks)
        xy, strength = self.chain_refine_batch(points, ranges, maps)
        measures = self.chain_measures(points, chains, strength=strength, xy=xy)
        if eps is None:
            return points, chains, ranges, xy, strength, measures
        return (points, chains, ranges, xy, strength, measures) + tuple(self.chain_polylines(points, chains, eps, return_index=True))

    def set_persist(self, on):
        """pipeline()/pipeline_batch(): keep the basis + orientation planes (default, like the reference
        object) or write the requested outputs only"""
        self._caller_check("set_persist")
        self.set_option(L.OPT_PERSIST_STATE, 1 if on else 0)

    def select_frame(self, i):
        self._caller_check("cvs_select_frame")
        self._check(lib().cvs_select_frame(self._h, int(i)), "cvs_select_frame")

    def _to_u8(self, plane, gain):
        self._caller_check("cvs_normalize_u8" if gain is None else "cvs_convert_u8")
        self._bind_stream(plane)
        pp = _plane(plane)
        if _is_torch(plane) and plane.is_cuda:
            dst = torch.empty(tuple(plane.shape), dtype=torch.uint8, device=plane.device)
            ptr, step, mem = C.c_void_p(dst.data_ptr()), dst.stride(0), L.MEM_DEVICE
        else:
            dst = np.empty(plane.shape, np.uint8)
            ptr, step, mem = C.c_void_p(dst.ctypes.data), dst.strides[0], L.MEM_HOST
        if gain is None:
            rc = lib().cvs_normalize_u8(self._h, C.byref(pp), ptr, step, mem)
        else:
            rc = lib().cvs_convert_u8(self._h, C.byref(pp), float(gain), 0.0, ptr, step, mem)
        self._check(rc, "cvs_normalize_u8" if gain is None else "cvs_convert_u8")
        return dst

    def normalize_u8(self, plane):
        """cv::normalize(plane, dst, 0, 255, NORM_MINMAX, CV_8UC1) on the GPU"""
        return self._to_u8(plane, None)

    def convert_u8(self, plane, gain):
        """plane.convertTo(dst, CV_8UC1, gain) on the GPU"""
        return self._to_u8(plane, gain)


class SteerableFiltersG2(_CallerPipeline, SteerableFilters):
    """fa::SteerableFiltersG2 (SteerableFiltersG2.h:35-67)."""

    KIND = L.KIND_G2
    DEFAULT_WIDTH = 4
    DEFAULT_SPACING = 0.67
    _DEFAULT_FLAGS = SETUP_FULL

    def getDominantOrientationAngle(self):
        return self._state(L.PLANE_THETA)

    def getDominantOrientationStrength(self):
        return self._state(L.PLANE_STRENGTH)

    def coefficients(self):
        """(C1, C2, C3) -- the reference's protected m_c1..m_c3"""
        return tuple(self._state(w) for w in (L.PLANE_C1, L.PLANE_C2, L.PLANE_C3))

    def steer_point(self, p, theta, full=False):
        """steer(const cv::Point& p, theta, ...): p = (x, y) = (col, row)"""
        out = (C.c_float * 5)()
        self._check(lib().cvs_steer_point(self._h, int(p[0]), int(p[1]), float(theta), out), "cvs_steer_point")
        vals = tuple(float(v) for v in out)
        return vals if full else vals[:2]

    def computeMagnitudeAndPhase(self, g2, h2):
        mag, phase = self._new_like(g2), self._new_like(g2)
        self._bind_stream(g2, h2, mag, phase)
        pg, ph, pm, pp = _plane(g2), _plane(h2), _plane(mag), _plane(phase)
        self._check(lib().cvs_mag_phase(self._h, C.byref(pg), C.byref(ph), C.byref(pm), C.byref(pp)), "cvs_mag_phase")
        return mag, phase

    def wrap(self, angle):
        """SteerableFilters::wrap (SteerableFilters.cpp:46-51)"""
        out = self._new_like(angle)
        self._bind_stream(angle, out)
        pa, po = _plane(angle), _plane(out)
        self._check(lib().cvs_wrap(self._h, C.byref(pa), C.byref(po)), "cvs_wrap")
        return out

    def phaseWeights(self, phase, phi, signum, k=2.0):
        lam = self._new_like(phase)
        self._bind_stream(phase, lam)
        pp, pl = _plane(phase), _plane(lam)
        self._check(lib().cvs_phase_weights(self._h, C.byref(pp), C.byref(pl), float(phi), int(bool(signum)), float(k)),
                    "cvs_phase_weights")
        return lam

class SteerableFiltersG4(_CallerPipeline, SteerableFilters):
    """fa::SteerableFiltersG4 (SteerableFiltersG4.h:35-57): setup + steer only.

    extensions=True switches on what the reference leaves unfinished (G4.h:55, G4.cpp:88-90): dominant
    orientation / strength / C1..C3 derived from the G4/H4 steering polynomials, steer(..., full=True)
    and a working computeMagnitudeAndPhase, and the callers' sequence of G2 -- find*, pipeline / pipeline_batch
    (outputs g4, h4, e, magnitude, phase, edges, dark, bright), set_persist, select_frame, normalize_u8 / convert_u8.
    Off by default: then the class behaves exactly like the reference (empty getters, no-op computeMagnitudeAndPhase)
    and the caller methods raise CvsError(E_UNSUPPORTED)."""

    KIND = L.KIND_G4
    DEFAULT_WIDTH = 6
    DEFAULT_SPACING = 0.5
    _DEFAULT_FLAGS = SETUP_BASIS

    def __init__(self, image=None, width=None, spacing=None, device=None, setup_flags=None, extensions=False):
        self.extensions = bool(extensions)
        super().__init__(None, width, spacing, device, setup_flags)
        if self.extensions:
            self.set_option(L.OPT_G4_EXTENSIONS, 1)
            if setup_flags is None:
                self._setup_flags = SETUP_FULL
        if image is not None:
            self.setup(image)

    def _caller_check(self, where):
        if not self.extensions:
            raise CvsError(L.E_UNSUPPORTED, where, "the G4 caller pipeline is an extension (extensions=True)")

    def getDominantOrientationAngle(self):
        """never assigned in the reference (G4.h:55): an empty Mat -- unless extensions are on"""
        return self._state(L.PLANE_THETA) if self.extensions else np.empty((0, 0), np.float32)

    def getDominantOrientationStrength(self):
        return self._state(L.PLANE_STRENGTH) if self.extensions else np.empty((0, 0), np.float32)

    def coefficients(self):
        if not self.extensions:
            raise CvsError(L.E_UNSUPPORTED, "coefficients", "G4 orientation is an extension (extensions=True)")
        return tuple(self._state(w) for w in (L.PLANE_C1, L.PLANE_C2, L.PLANE_C3))

    def computeMagnitudeAndPhase(self, g4, h4, magnitude=None, phase=None):
        """empty body in the reference (G4.cpp:88-90): outputs untouched -- unless extensions are on"""
        if not self.extensions:
            return magnitude, phase
        mag, ph = self._new_like(g4), self._new_like(g4)
        self._bind_stream(g4, h4, mag, ph)
        pg, phh, pm, pp = _plane(g4), _plane(h4), _plane(mag), _plane(ph)
        self._check(lib().cvs_mag_phase(self._h, C.byref(pg), C.byref(phh), C.byref(pm), C.byref(pp)), "cvs_mag_phase")
        return mag, ph
