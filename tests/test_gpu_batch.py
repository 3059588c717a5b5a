"""GPU tests (-m gpu): the native batch layer (cvs_batch_*, cvsteer_amd/csrc/cvs_batch.cpp) -- the batch axis of
example/steer.cpp:69-124,169 and the row-band split of one large image / pyramid.

A gpurun box has ONE GPU, so:
  * RCCL itself is exercised in a one-rank world (ncclCommInitAll / ncclCommInitRank with 1 rank): with
    self_via_transport the root's block really travels through grouped ncclSend / ncclRecv, and the pyramid issues
    its ncclBroadcast;
  * the N > 1 bookkeeping (sharding, staging, ordering, band seams, empty shards) runs with several ranks sharing
    device 0, where the library switches to its rehearsal transport (stream-ordered device copies);
  * a two-PROCESS world with the HIP engine as the frame function runs over torch.distributed / gloo.
Everything is checked bit for bit against the single-handle engine (which tests/test_gpu_parity.py pins to the oracle).
"""
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cv():
    import cvsteer_amd
    return cvsteer_amd


def _frames(n, rows, cols, seed):
    import torch
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand((n, rows, cols), device="cuda", generator=gen)


def _reference(cv, frames, sel):
    eng = cv.SteerableFiltersG2(None)
    return eng.pipeline_batch(frames, outputs=sel)


@pytest.mark.parametrize("via", [False, True])
def test_one_rank_world_rccl(cv, via):
    import torch
    from cvsteer_amd import batch
    frames = _frames(5, 70, 200, 3)
    want = _reference(cv, frames, (5, 6, 7))
    nb = batch.NativeBatch.local((0,))
    assert nb.transport in ("rccl", "none")
    if via and nb.transport != "rccl":
        pytest.skip("RCCL could not be loaded on this box")
    got, t = nb.run(frames, 5, (70, 200), outputs=(5, 6, 7), self_via_transport=via)
    assert torch.equal(got, want)
    assert t["compute"] > 0.0
    # all eight outputs, a second call on the same object (staging reuse), other geometry
    frames2 = _frames(3, 129, 513, 4)
    got2, _ = nb.run(frames2, 3, (129, 513), outputs=tuple(range(8)), self_via_transport=via)
    assert torch.equal(got2, _reference(cv, frames2, tuple(range(8))))
    nb.close()


def test_rank_per_process_bootstrap_one_rank(cv):
    """cvs_batch_unique_id + cvs_batch_create_rank (the one-process-per-GPU way to form a world), here with one rank"""
    import torch
    from cvsteer_amd import batch
    try:
        nb = batch.NativeBatch.from_torch_distributed(0)
    except cv.CvsError as e:
        pytest.skip("RCCL not available: %s" % e)
    assert nb.world == 1 and nb.transport == "rccl"
    frames = _frames(4, 64, 128, 9)
    got, _ = nb.run(frames, 4, (64, 128), outputs=(0, 1, 7), self_via_transport=True)
    assert torch.equal(got, _reference(cv, frames, (0, 1, 7)))
    nb.close()


@pytest.mark.parametrize("world,n_frames", [(2, 5), (3, 7), (3, 2), (4, 1), (8, 32)])
def test_rehearsal_world_sharded_equals_unsharded(cv, world, n_frames):
    """several ranks on device 0: contiguous blocks, empty shards, root in place, gather order"""
    import torch
    from cvsteer_amd import batch
    rows, cols = (1080 // 8, 1920 // 8) if n_frames == 32 else (48, 136)
    frames = _frames(n_frames, rows, cols, 10 + world)
    want = _reference(cv, frames, (2, 5, 6, 7))
    nb = batch.NativeBatch.local((0,) * world)
    assert nb.transport.startswith("device copies")
    got, t = nb.run(frames, n_frames, (rows, cols), outputs=(2, 5, 6, 7))
    assert torch.equal(got, want)
    # a root other than rank 0
    if world > 1:
        got_r, _ = nb.run(frames, n_frames, (rows, cols), outputs=(2, 5, 6, 7), root=world - 1)
        assert torch.equal(got_r, want)
    nb.close()


@pytest.mark.parametrize("world,n_frames,persist", [(1, 6, False), (1, 3, True), (3, 11, False), (4, 2, False), (2, 9, True)])
def test_host_planes_every_rank_pulls_its_own_frames(cv, world, n_frames, persist):
    """cvs_batch_run with HOST planes (example/steer.cpp:73-104 holds cv::Mat): ranks upload their frames themselves,
    chunked and overlapped with the launches and the downloads; padded host rows; results bit-identical"""
    import torch
    from cvsteer_amd import batch
    rows, cols = 90, 333
    frames = _frames(n_frames, rows, cols, 17)
    want = _reference(cv, frames, (0, 4, 5, 6, 7)).cpu().numpy()
    padded = np.full((n_frames, rows, cols + 13), np.nan, np.float32)   # host rows with padding behind them
    padded[:, :, :cols] = frames.cpu().numpy()
    host = padded[:, :, :cols]
    nb = batch.NativeBatch.local((0,) * world)
    nb.set_persist(persist)
    got, t = nb.run(host, n_frames, (rows, cols), outputs=(0, 4, 5, 6, 7))
    assert isinstance(got, np.ndarray) and np.array_equal(got, want)
    assert t["scatter"] > 0 and t["gather"] > 0 and t["compute"] >= t["gather"]
    # again into a caller-owned array, other selection
    out = np.zeros((n_frames, 2, rows, cols), np.float32)
    got2, _ = nb.run(host, n_frames, (rows, cols), outputs=(5, 7), out=out)
    assert got2 is out and np.array_equal(out[:, 0], want[:, 2]) and np.array_equal(out[:, 1], want[:, 4])
    # host in, device out is not a defined mix
    dev_out = torch.empty((n_frames, 3, rows, cols), device="cuda")
    with pytest.raises(AssertionError):
        nb.run(host, n_frames, (rows, cols), out=dev_out)
    nb.close()


def test_to_u8_batch_equals_plane_by_plane(cv):
    """cvs_normalize_u8_batch / cvs_convert_u8_batch (steer.cpp:92-98 for a whole block of maps): one launch pair and one
    sync for n planes, bit-identical to the single-plane calls; irregular plane lists fall back to plane by plane"""
    import ctypes as C
    import torch
    from cvsteer_amd import _lib as L
    lib = L.lib()
    eng = cv.SteerableFiltersG2(None)
    n, rows, cols = 7, 61, 300
    gen = torch.Generator(device="cuda").manual_seed(2)
    block = (torch.rand((n, rows, cols), device="cuda", generator=gen) - 0.3) * torch.arange(1, n + 1, device="cuda").view(n, 1, 1) * 40.0
    block[3] = 5.0                                     # a constant plane: max == min
    want_n = torch.stack([eng.normalize_u8(block[i]) for i in range(n)]).cpu().numpy()
    want_c = torch.stack([eng.convert_u8(block[i], 1.7) for i in range(n)]).cpu().numpy()

    def planes_of(t):
        arr = (L.Plane * len(t))()
        for i, x in enumerate(t):
            arr[i] = L.Plane(x.data_ptr(), rows, cols, x.stride(0) * 4, L.MEM_DEVICE)
        return arr

    scattered = [block[i].clone() if i % 2 else block[i] for i in range(n)]                # kept alive for the calls below
    for src in (planes_of([block[i] for i in range(n)]),                                   # regular: one launch pair
                planes_of(scattered)):                                                     # irregular: fallback
        host = np.zeros((n, rows, cols + 5), np.uint8)
        dst = (C.c_void_p * n)(*[host[i].ctypes.data for i in range(n)])
        assert lib.cvs_normalize_u8_batch(eng._h, src, n, dst, cols + 5, L.MEM_HOST) == 0
        assert np.array_equal(host[:, :, :cols], want_n) and not host[:, :, cols:].any()
        assert lib.cvs_convert_u8_batch(eng._h, src, n, C.c_float(1.7), C.c_float(0.0), dst, cols + 5, L.MEM_HOST) == 0
        assert np.array_equal(host[:, :, :cols], want_c)
        dev = torch.zeros((n, rows, cols), dtype=torch.uint8, device="cuda")
        ddst = (C.c_void_p * n)(*[dev[i].data_ptr() for i in range(n)])
        assert lib.cvs_normalize_u8_batch(eng._h, src, n, ddst, cols, L.MEM_DEVICE) == 0
        lib.cvs_sync(eng._h)
        assert np.array_equal(dev.cpu().numpy(), want_n)
    assert lib.cvs_normalize_u8_batch(eng._h, src, 0, dst, cols, L.MEM_HOST) == L.E_BADARG


def test_pipeline_batch_widens_a_block_of_byte_frames_in_one_launch(cv):
    """8-bit frames lying back to back on the device (a driver's upload) take the one-launch path: same results as f32"""
    import ctypes as C
    import torch
    from cvsteer_amd import _lib as L
    lib = L.lib()
    n, rows, cols = 5, 130, 257
    gen = torch.Generator(device="cuda").manual_seed(9)
    u8 = (torch.rand((n, rows, cols), device="cuda", generator=gen) * 255).to(torch.uint8).contiguous()
    want = cv.SteerableFiltersG2(None).pipeline_batch(u8.to(torch.float32), outputs=(3, 4, 5, 6, 7))
    eng = cv.SteerableFiltersG2(None)
    out = torch.zeros((n, 5, rows, cols), device="cuda")
    ims = (L.Plane * n)()
    outs = (L.Plane * (n * 8))()
    for i in range(n):
        ims[i] = L.Plane(u8[i].data_ptr(), rows, cols, cols, L.MEM_DEVICE | L.DEPTH_U8)
        for j, k in enumerate((3, 4, 5, 6, 7)):
            outs[i * 8 + k] = L.Plane(out[i, j].data_ptr(), rows, cols, cols * 4, L.MEM_DEVICE)
    assert lib.cvs_pipeline_batch(eng._h, ims, n, outs) == 0
    lib.cvs_sync(eng._h)
    assert torch.equal(out, want)
    eng.select_frame(n - 1)                     # state of every frame is there, as after an f32 batch
    single = cv.SteerableFiltersG2(u8[n - 1].to(torch.float32))
    eng._like = out                                # results as CUDA tensors (the raw ctypes call above did not say)
    assert torch.equal(eng.basis(2), single.basis(2))


@pytest.mark.parametrize("world", [1, 3])
def test_byte_frames_from_host_and_the_whole_driver_flow(cv, world):
    """uint8 host frames through cvs_batch_run (bytes cross the link) == float frames; NativeBatch.run_to_u8 (maps kept on the
    GPUs, converted there, only bytes come back) == the single-engine pipeline + normalize_u8 / convert_u8 per plane"""
    import torch
    from cvsteer_amd import batch
    n, rows, cols = 7, 75, 210
    rng = np.random.default_rng(11)
    u8 = rng.integers(0, 256, (n, rows, cols), dtype=np.uint8)
    nb = batch.NativeBatch.local((0,) * world)
    nb.set_persist(False)
    got_b, _ = nb.run(u8, n, (rows, cols), outputs=(5, 6, 7))
    got_f, _ = nb.run(u8.astype(np.float32), n, (rows, cols), outputs=(5, 6, 7))
    assert np.array_equal(got_b, got_f)
    eng = cv.SteerableFiltersG2(None)
    ref = eng.pipeline_batch(torch.from_numpy(u8.astype(np.float32)).cuda(), outputs=(5, 6, 7))
    assert np.array_equal(got_b, ref.cpu().numpy())
    q, _ = nb.run_to_u8(u8)
    want = torch.stack([torch.stack([eng.normalize_u8(ref[i, j]) for j in range(3)]) for i in range(n)]).cpu().numpy()
    assert q.dtype == np.uint8 and np.array_equal(q, want)
    q2, _ = nb.run_to_u8(u8.astype(np.float32), gain=3.0)
    want2 = torch.stack([torch.stack([eng.convert_u8(ref[i, j], 3.0) for j in range(3)]) for i in range(n)]).cpu().numpy()
    assert np.array_equal(q2, want2)
    # the one-call flow (8-bit host output planes of cvs_batch_run, chunks overlapped) == the two-step flow, with the
    # state kept (one chunk) and without, and for a single requested map
    for persist in (False, True):
        nb.set_persist(persist)
        a1, _ = nb.run_to_u8(u8)
        a2, _ = nb.run_to_u8_two_step(u8)
        assert np.array_equal(a1, want) and np.array_equal(a2, want)
        b1, _ = nb.run_to_u8(u8, outputs=(6,), gain=1.5)
        b2, _ = nb.run_to_u8_two_step(u8, outputs=(6,), gain=1.5)
        assert np.array_equal(b1, b2)
    nb.close()


def test_host_planes_mixed_with_device_planes_rejected(cv):
    import ctypes as C
    from cvsteer_amd import _lib as L
    lib = L.lib()
    h = C.c_void_p()
    devs = (C.c_int * 1)(0)
    assert lib.cvs_batch_create_local(L.KIND_G2, 4, C.c_float(0.67), 1, devs, C.byref(h)) == 0
    import torch
    img = np.random.default_rng(0).random((40, 64), dtype=np.float32)
    dev = torch.zeros((40, 64), device="cuda")
    ins = (L.Plane * 1)(L.Plane(img.ctypes.data, 40, 64, 64 * 4, L.MEM_HOST))
    outs = (L.Plane * 8)()
    outs[5] = L.Plane(dev.data_ptr(), 40, 64, 64 * 4, L.MEM_DEVICE)
    cfg = L.BatchCfg(40, 64, 1, 1 << 5, 0, 1, 0)
    rc = lib.cvs_batch_run(h, C.byref(cfg), ins, outs, None)
    assert rc == L.E_SIZE and b"host" in lib.cvs_batch_last_error(h)
    lib.cvs_batch_destroy(h)


@pytest.mark.parametrize("world", [1, 3])
def test_byte_output_planes_padded_and_mixed_rejected(cv, world):
    """cvs_batch_run with 8-bit HOST output planes through the C ABI: padded rows (step > cols) and planes that do not lie
    back to back take the per-plane copies and give the same bytes; f32 and 8-bit output planes in one call are refused"""
    import ctypes as C
    import torch
    from cvsteer_amd import _lib as L
    from cvsteer_amd import batch
    n, rows, cols = 5, 61, 130
    u8 = np.random.default_rng(3).integers(0, 256, (n, rows, cols), dtype=np.uint8)
    nb = batch.NativeBatch.local((0,) * world)
    nb.set_persist(False)
    want, _ = nb.run_to_u8(u8)                      # dense [n][3][rows][cols] block: linear copies
    lib = L.lib()
    pad = np.full((n, 3, rows, cols + 14), 7, np.uint8)
    ins = (L.Plane * n)(*[L.Plane(u8[i].ctypes.data, rows, cols, cols, L.MEM_HOST | L.DEPTH_U8) for i in range(n)])
    outs = (L.Plane * (8 * n))()
    for i in range(n):
        for j, k in enumerate((5, 6, 7)):
            outs[i * 8 + k] = L.Plane(pad[i, j].ctypes.data, rows, cols, cols + 14, L.MEM_HOST | L.DEPTH_U8)
    cfg = L.BatchCfg(rows, cols, n, (1 << 5) | (1 << 6) | (1 << 7), 0, 1, 0)
    assert lib.cvs_batch_set_u8_gain(nb._b, C.c_float(0.0)) == 0
    assert lib.cvs_batch_run(nb._b, C.byref(cfg), ins, outs, None) == 0, lib.cvs_batch_last_error(nb._b)
    assert np.array_equal(pad[..., :cols], want) and (pad[..., cols:] == 7).all()
    # one f32 plane among the 8-bit ones
    f32 = np.zeros((rows, cols), np.float32)
    outs[6] = L.Plane(f32.ctypes.data, rows, cols, cols * 4, L.MEM_HOST)
    assert lib.cvs_batch_run(nb._b, C.byref(cfg), ins, outs, None) == L.E_SIZE
    assert lib.cvs_batch_set_u8_gain(nb._b, C.c_float(-1.0)) == L.E_BADARG
    nb.close()


@pytest.mark.parametrize("persist", [False, True])
@pytest.mark.parametrize("world", [1, 3])
def test_host_planes_runs_that_break_and_continue(cv, world, persist):
    """cvs_batch_run through the C ABI with host planes that make the copy coalescer work: input frames in slots 0 1 | 3 4 5 | 8 9 10 11 12
    of one [15] block (dense runs of 2, 3 and 5) and an eleventh frame with padded rows in an array of its own; the three output maps in
    slots 0 1 | 3 of an [n][4] block, so that a run breaks after two planes inside a frame and continues from slot 3 into slot 0 of the next
    frame, one plane of a middle frame redirected to a padded array.  With three ranks the shards are 4 | 4 | 3 frames, and without kept
    state a shard of 4 runs as chunks 1 | 3: runs are cut at chunk boundaries too.  f32 in / f32 out and 8-bit in / 8-bit out (normalised,
    and gain 3.0): bit-identical to the same frames as one dense block, every byte around the planes untouched."""
    import ctypes as C
    from cvsteer_amd import _lib as L
    from cvsteer_amd import batch
    lib = L.lib()
    n, rows, cols, sel = 11, 33, 70, (5, 6, 7)
    in_slots, out_slots, moved = (0, 1, 3, 4, 5, 8, 9, 10, 11, 12), (0, 1, 3), (5, 1)
    rng = np.random.default_rng(23)
    nb = batch.NativeBatch.local((0,) * world)
    nb.set_persist(persist)
    cfg = L.BatchCfg(rows, cols, n, sum(1 << k for k in sel), 0, 1, 0)
    for dtype, gains in ((np.float32, (None,)), (np.uint8, (0.0, 3.0))):
        u8 = dtype == np.uint8
        esz, mem = (1, L.MEM_HOST | L.DEPTH_U8) if u8 else (4, L.MEM_HOST)
        dense = rng.integers(0, 256, (n, rows, cols), dtype=np.uint8) if u8 else rng.random((n, rows, cols), dtype=np.float32)
        in_mark, out_mark = (0xEE, 0x5A) if u8 else (np.nan, np.nan)
        block = np.full((15, rows, cols), in_mark, dtype)
        block[list(in_slots)] = dense[:10]
        own = np.full((rows, cols + 9), in_mark, dtype)
        own[:, :cols] = dense[10]
        block_before, own_before = block.tobytes(), own.tobytes()
        ins = (L.Plane * n)(*([L.Plane(block[k].ctypes.data, rows, cols, cols * esz, mem) for k in in_slots] +
                             [L.Plane(own.ctypes.data, rows, cols, (cols + 9) * esz, mem)]))
        for gain in gains:
            want = nb.run_to_u8(dense, outputs=sel, gain=gain)[0] if u8 else nb.run(dense, n, (rows, cols), outputs=sel)[0]
            oblock = np.full((n, 4, rows, cols), out_mark, dtype)
            opad = np.full((rows, cols + 11), out_mark, dtype)
            outs = (L.Plane * (8 * n))()
            for i in range(n):
                for j, k in enumerate(sel):
                    outs[i * 8 + k] = L.Plane(oblock[i, out_slots[j]].ctypes.data, rows, cols, cols * esz, mem)
            outs[moved[0] * 8 + sel[moved[1]]] = L.Plane(opad.ctypes.data, rows, cols, (cols + 11) * esz, mem)
            if u8:
                assert lib.cvs_batch_set_u8_gain(nb._b, C.c_float(gain)) == 0
            t = L.BatchTiming()
            assert lib.cvs_batch_run(nb._b, C.byref(cfg), ins, outs, C.byref(t)) == 0, lib.cvs_batch_last_error(nb._b)
            untouched = (lambda a: bool(np.isnan(a).all())) if not u8 else (lambda a: bool((a == out_mark).all()))
            for i in range(n):
                for j in range(3):
                    if (i, j) == moved:
                        assert np.array_equal(opad[:, :cols], want[i, j]) and untouched(opad[:, cols:]) and untouched(oblock[i, out_slots[j]])
                    else:
                        assert np.array_equal(oblock[i, out_slots[j]], want[i, j]), (i, j)
            assert untouched(oblock[:, 2])
            assert block.tobytes() == block_before and own.tobytes() == own_before
            assert t.scatter_ms > 0 and t.gather_ms > 0 and t.compute_ms >= t.gather_ms
    nb.close()


_AGREE_SCRIPT = r"""
import ctypes as C, sys, torch
import cvsteer_amd as cv
from cvsteer_amd import batch, _lib as L
try:
    nb = batch.NativeBatch.from_torch_distributed(0)
except cv.CvsError as e:
    print("SKIP", e); sys.exit(0)
assert nb.transport == "rccl"
gen = torch.Generator(device="cuda").manual_seed(3)
frames = torch.rand((5, 70, 200), device="cuda", generator=gen)
want = cv.SteerableFiltersG2(None).pipeline_batch(frames, outputs=(5, 6, 7))
got, t = nb.run(frames, 5, (70, 200), outputs=(5, 6, 7), self_via_transport=True)     # agreement, then scatter / compute / gather
assert torch.equal(got, want)
# a root-only failure is an ERROR RETURN after the agreement (nothing queued, the group closed), and the object stays usable
bad = torch.rand((5, 70, 256), device="cuda", generator=gen)[:, :, :200]               # padded rows: not dense planes
imgs = (L.Plane * 5)(*[L.Plane(bad[i].data_ptr(), 70, 200, 256 * 4, L.MEM_DEVICE) for i in range(5)])
outs = (L.Plane * 40)()
cfg = L.BatchCfg(70, 200, 5, 0xE0, 0, 1, 0)
tm = L.BatchTiming()
rc = L.lib().cvs_batch_run(nb._b, C.byref(cfg), imgs, outs, C.byref(tm))
assert rc == L.E_SIZE, rc
got2, _ = nb.run(frames, 5, (70, 200), outputs=(5, 6, 7))
assert torch.equal(got2, want)
img = torch.rand((300, 400), device="cuda", generator=gen)
nb.pyramid_setup(img, 300, 400, 3, flags=cv.SETUP_BASIS)
assert torch.equal(nb.level_plane(0, L.PLANE_BASIS0 + 2), cv.SteerableFiltersG2(img).basis(2))
nb.close()
print("AGREE_OK")
"""


def test_status_agreement_path_runs_in_a_one_rank_world(tmp_path):
    """cvs_batch.cpp agree(): ranks of a multi-process world all-reduce {status, geometry hash} before anything is queued.
    With CVS_BATCH_FORCE_AGREE=1 a one-rank RCCL world goes through the same code (device scratch, grouped ncclAllReduce,
    readback), the only way to exercise it on a one-GPU box; a root-side validation failure comes back as an error return
    with the group closed and the batch still usable."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CVS_BATCH_FORCE_AGREE="1", CVS_BATCH_SELF_TRANSPORT="1", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", _AGREE_SCRIPT], env=env, capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    if "SKIP" in r.stdout:
        pytest.skip("RCCL not available: " + r.stdout)
    assert "AGREE_OK" in r.stdout


def test_batch_argument_errors(cv):
    import torch
    from cvsteer_amd import batch
    nb = batch.NativeBatch.local((0,))
    frames = _frames(2, 32, 64, 1)
    with pytest.raises(cv.CvsError):
        nb.run(frames, 2, (32, 64), outputs=())             # nothing requested
    with pytest.raises(cv.CvsError):
        nb.run(frames, 2, (32, 64), root=3)                 # no such rank
    with pytest.raises(cv.CvsError):
        batch.NativeBatch.local((0, 99))                    # no such device
    nb.close()


@pytest.mark.parametrize("world", [1, 3, 4])
def test_pyramid_bands_equal_single_gpu(cv, world, monkeypatch):
    """config 3: broadcast + row bands of every level + gather into the root's state == one GPU, bit for bit
    (band seams, image borders, odd level sizes, a level with fewer rows than a strip)"""
    import torch
    from cvsteer_amd import _lib as L
    from cvsteer_amd import batch
    if world == 1:
        monkeypatch.setenv("CVS_BATCH_SELF_TRANSPORT", "1")   # the one-rank world still issues ncclBroadcast
    rows, cols, levels = 523, 777, 5
    gen = torch.Generator(device="cuda").manual_seed(21)
    img = torch.rand((rows, cols), device="cuda", generator=gen)
    single = cv.SteerableFiltersG2(None)
    lv = single.pyramid(img, levels)
    nb = batch.NativeBatch.local((0,) * world)
    t = nb.pyramid_setup(img, rows, cols, levels, flags=cv.SETUP_FULL)
    assert t["compute"] > 0.0
    for l, plane in enumerate(lv):
        ref = cv.SteerableFiltersG2(plane)
        for p in range(7):
            assert torch.equal(nb.level_plane(l, L.PLANE_BASIS0 + p), ref.basis(p)), (l, p)
        assert torch.equal(nb.level_plane(l, L.PLANE_THETA), ref.getDominantOrientationAngle()), l
        assert torch.equal(nb.level_plane(l, L.PLANE_C1), ref.coefficients()[0]), l
    nb.close()
    # G4 basis planes through the same path
    nb4 = batch.NativeBatch.local((0,) * world, kind=L.KIND_G4, width=6, spacing=0.5)
    nb4.pyramid_setup(img, rows, cols, 3, flags=cv.SETUP_BASIS)
    for l in range(3):
        ref = cv.SteerableFiltersG4(lv[l])
        for p in (0, 5, 10):
            assert torch.equal(nb4.level_plane(l, L.PLANE_BASIS0 + p), ref.basis(p)), (l, p)
    nb4.close()


def test_two_distinct_devices_rccl_round_trip(cv):
    """the batch axis of example/steer.cpp:169 over RCCL between DISTINCT devices -- runs wherever two GPUs are visible (the driver's 8-GPU
    node; a one-GPU box skips): 1080p frames scattered from device 0 with grouped ncclSend / ncclRecv, one fused launch per device, the
    three maps gathered back, bit for bit the single-GPU result; then one banded pyramid (ncclBroadcast of the image, row bands of every
    level per device, bands gathered into the root's planes) against the single-GPU chain, band seams included"""
    import torch
    from cvsteer_amd import _lib as L
    from cvsteer_amd import batch
    ndev = torch.cuda.device_count()
    if ndev < 2:
        pytest.skip("one GPU visible: RCCL between distinct devices cannot run here")
    devs = tuple(range(min(ndev, 4)))
    frames = _frames(len(devs) + 1, 1080, 1920, 31)          # an uneven split: one device gets two frames
    want = _reference(cv, frames, (5, 6, 7))
    nb = batch.NativeBatch.local(devs)
    assert nb.transport == "rccl", nb.transport              # a rehearsal transport must never carry distinct devices
    got, t = nb.run(frames, frames.shape[0], (1080, 1920), outputs=(5, 6, 7))
    assert torch.equal(got, want)
    assert t["scatter"] > 0.0 and t["compute"] > 0.0 and t["gather"] > 0.0
    got8, _ = nb.run(frames, frames.shape[0], (1080, 1920), outputs=tuple(range(8)))
    assert torch.equal(got8, _reference(cv, frames, tuple(range(8))))
    rows, cols, levels = 2051, 3000, 4
    img = torch.rand((rows, cols), device="cuda", generator=torch.Generator(device="cuda").manual_seed(32))
    single = cv.SteerableFiltersG2(None)
    lv = single.pyramid(img, levels)
    tp = nb.pyramid_setup(img, rows, cols, levels, flags=cv.SETUP_FULL)
    assert tp["broadcast"] > 0.0 and tp["gather"] > 0.0
    for l, plane in enumerate(lv):
        ref = cv.SteerableFiltersG2(plane)
        for p in range(7):
            assert torch.equal(nb.level_plane(l, L.PLANE_BASIS0 + p), ref.basis(p)), (l, p)
        assert torch.equal(nb.level_plane(l, L.PLANE_THETA), ref.getDominantOrientationAngle()), l
    nb.close()


def test_setup_rows_band_is_bit_identical(cv):
    """cvs_setup_rows: any band of rows equals the same rows of a whole-image setup, incl. bands touching the borders"""
    import ctypes as C
    import torch
    img = torch.rand((300, 333), device="cuda")
    whole = cv.SteerableFiltersG2(img)
    for lo, hi in ((0, 300), (0, 7), (5, 6), (100, 181), (293, 300)):
        f = cv.SteerableFiltersG2(None)
        f._like = img                  # results as CUDA tensors
        f._bind_stream(img)
        p = cv.api._plane(img)
        f._check(cv.lib().cvs_setup_rows(f._h, C.byref(p), cv.SETUP_FULL, lo, hi), "cvs_setup_rows")
        for k in (0, 3, 6):
            assert torch.equal(f.basis(k)[lo:hi], whole.basis(k)[lo:hi]), (lo, hi, k)
        assert torch.equal(f.getDominantOrientationAngle()[lo:hi], whole.getDominantOrientationAngle()[lo:hi])
    f = cv.SteerableFiltersG2(None)
    p = cv.api._plane(img)
    with pytest.raises(cv.CvsError):
        f._check(cv.lib().cvs_setup_rows(f._h, C.byref(p), cv.SETUP_FULL, 10, 10), "cvs_setup_rows")


# ------------------------------------------------------------------ two processes, the HIP engine as the frame function
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, n_frames, q):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import torch.distributed as dist
    import cvsteer_amd as cv
    from cvsteer_amd import batch
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)   # both ranks share the box's one GPU; gloo carries the frames through host memory
        shape = (96, 160)
        frames = None
        if rank == 0:
            frames = torch.from_numpy(np.random.default_rng(5).random((n_frames,) + shape, dtype=np.float32))
        eng = cv.SteerableFiltersG2(None, device=0)

        def frame_fn(img, outs):   # the product's frame function: the HIP pipeline, nothing else
            res = eng.pipeline(img.cuda())
            for o, r in zip(outs, res):
                o.copy_(r)

        local, gathered = batch.run_sharded(frames, n_frames, shape, torch.device("cpu"), frame_fn, 8)
        lo, hi = batch.shard_range(n_frames, world, rank)
        assert local.shape == (hi - lo, 8) + shape
        if rank == 0:
            want = cv.SteerableFiltersG2(None, device=0).pipeline_batch(frames.cuda()).cpu()
            assert gathered.shape == want.shape
            assert torch.equal(gathered, want)   # sharded over two processes == one launch, bit for bit
            q.put("ok")
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("n_frames", [5, 1])
def test_two_processes_hip_frame_function(n_frames):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, n_frames, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert q.get(timeout=5) == "ok"


def _json_line(stdout):
    import json
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, stdout[-2000:]
    return json.loads(lines[0])


def test_bench_starts_its_own_ranks_and_watchdog_emits_the_headline(tmp_path):
    """bench.py --gpus 2 without a launcher: the parent starts two rank processes before it touches the GPU (rehearsal on one
    device: CVS_BENCH_TEST_BACKEND=gloo puts both ranks on device 0), rank 0 prints ONE JSON line with n_gpus = 2; and with
    a watchdog too short for the secondary legs the line still carries the headline + extra_error -- and the exit status is
    NOT zero (a hung set of secondary legs must not look like a clean run)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CVS_BENCH_TEST_BACKEND="gloo")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--full", "--gpus", "2", "--steps", "5", "--warmup", "2", "--no-extra", "--repeats", "3"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _json_line(r.stdout)
    assert d["n_gpus"] == 2 and d["steps"] == 5 and d["value"] > 0 and d["config"]["ranks_started_by"] == "bench.py"
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and 0 < rf["frac"] < 1.2
    assert d["config"]["repeats"] == 3 and d["config"]["Mpix_s_min"] <= d["value"] <= d["config"]["Mpix_s_max"]
    # the headline runs on the library's defaults; everything the driver must see sits in `roofline` as flat scalars
    assert d["config"]["library_defaults"] is True
    nested = {"m1", "fresh", "one_object", "first_call", "after_idle"}     # the same figures once more as roofline.m1.frac ... (the form the round-4 verdict named)
    assert all(not isinstance(v, (dict, list)) for k, v in rf.items() if k not in nested), rf
    assert all(isinstance(rf[k], dict) and all(not isinstance(v, (dict, list)) for v in rf[k].values()) for k in nested if k in rf), rf
    assert rf["m1"]["frac"] == rf["m1_frac"] and all(rf[k]["frac"] == rf[k + "_frac"] for k in nested - {"m1"} if k in rf)
    assert all(not isinstance(v, (dict, list)) for v in d["config"].values()) and all(not isinstance(v, (dict, list)) for v in d["cpu_baseline"].values())
    assert 0 < rf["m1_frac"] < 1.2 and rf["m1_ms_min"] <= rf["m1_ms"] <= rf["m1_ms_max"]      # north_star's own target, inside the kept dict
    cfg = d["launch_configs"][d["config"]["launch_config"]]
    assert cfg[3] == 1 and len(cfg) == 7 and cfg[5] == 3                                        # row-interleaved state; the fused steer at three workgroups per CU
    assert d["legs"]["M1_basis"][0] == rf["m1_frac"]
    assert rf["rccl_ranks"] == 0 and d["config"]["distinct_devices"] is False                 # rehearsal on one GPU
    assert "cpu_baseline" in d and d["cpu_baseline"]["kind"] == "port"        # rank 0 measures it for N > 1 as well
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--full", "--steps", "5", "--warmup", "2", "--no-cpu", "--extra-timeout", "1", "--repeats", "3"],
                       env=os.environ, capture_output=True, text=True, timeout=600)
    assert r.returncode == 3, (r.returncode, r.stderr[-2000:])
    d = _json_line(r.stdout)
    assert d["n_gpus"] == 1 and d["value"] > 0 and "watchdog" in d["extra_error"]


def test_bench_dump_outputs_are_what_the_timed_call_returns(tmp_path):
    """bench.py --dump-outputs DIR: DIR/g.npy and DIR/h.npy are the rows bench._dump_rows() names of the g / h the headline call
    (setup_steer of the seeded 4096^2 image at theta 0.3) returns, bit for bit; the line carries --steps and ms_per_step."""
    import importlib.util
    import subprocess
    import sys
    import torch
    import cvsteer_amd as cv
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "4", "--warmup", "2", "--repeats", "2", "--no-extra", "--no-cpu",
                        "--no-live-traffic", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = _json_line(r.stdout)
    assert line["steps"] == 4 and line["ms_per_step"] > 0 and line["dump_outputs"] == str(d)
    assert sorted(os.listdir(d)) == ["g.npy", "h.npy"]
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    img = torch.rand((bench.ROWS, bench.COLS), generator=torch.Generator(device="cuda").manual_seed(1234), device="cuda", dtype=torch.float32)
    g, h = cv.SteerableFiltersG2(None, 4, 0.67).setup_steer(img, bench.THETA, flags=cv.SETUP_BASIS)
    rows = bench._dump_rows()
    for name, want in (("g", g), ("h", h)):
        got = np.load(d / (name + ".npy"))
        assert got.dtype == np.float32 and got.shape == (len(rows), bench.COLS)
        assert np.array_equal(got, want.cpu().numpy()[rows]), name


def test_bench_plain_run_is_the_headline_alone(tmp_path):
    """bench.py without --full: the headline and nothing else -- no M1, no secondary legs, no CPU baseline, no counter passes --
    and the contract keys as a --full run carries them; the whole process stays well inside the 30 s a plain run may spend
    outside its steps."""
    import subprocess
    import sys
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "5", "--warmup", "2"],
                       capture_output=True, text=True, timeout=600)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    d = _json_line(r.stdout)
    assert d["metric"].startswith("Mpix/s for G2+H2") and d["unit"] == "Mpix/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["steps"] == 5 and d["warmup"] == 2
    assert d["config"]["full"] is False and d["config"]["repeats"] == 15
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and 0 < rf["frac"] < 1.2 and rf["avg_launch_ms"] > 0
    assert "legs" not in d and "m1_frac" not in rf and "sclk_mhz" not in rf and d["cpu_baseline"] is None and "extra_error" not in d
    assert "traffic_read_bytes" not in rf                                   # the live counter passes did not run
    assert wall < 30, wall


def test_bench_two_ranks_with_the_secondary_legs_and_a_crashing_rank(tmp_path):
    """the N > 1 rehearsal WITH the secondary legs (round-2 verdict: the rehearsal passed --no-extra): both ranks on device 0,
    gloo for the collectives, every leg that does not need an RCCL communicator runs with its barriers and its
    max-over-ranks reductions; then the same with rank 1 dying inside the legs -- the parent stops rank 0 with SIGTERM, whose
    watcher thread still prints the line (headline + extra_error), and the parent's status is non-zero."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CVS_BENCH_TEST_BACKEND="gloo")
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--full", "--gpus", "2", "--steps", "3", "--warmup", "1", "--repeats", "3", "--leg-repeats", "1", "--no-cpu"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _json_line(r.stdout)
    assert d["n_gpus"] == 2 and "extra_error" not in d
    lg, rf = d["legs"], d["roofline"]
    for name in ("M1_basis", "M2_fresh_8_rotating", "M2_one_object_per_image", "M2_first_call_synchronised", "M2_after_idle",
                 "C4_32x1080p_pipeline_state_kept", "C4_32x1080p_three_maps_only"):
        assert name in lg and lg[name][1] > 0, (name, lg.get(name))
    for key in ("fresh_frac", "one_object_frac", "first_call_frac", "after_idle_frac", "c4_frac"):
        assert 0 < rf[key] < 1.2, (key, rf.get(key))
    assert len(r.stdout.strip()) < 6144, len(r.stdout)        # the whole line fits the driver's 8 KB tail with room to spare
    r = subprocess.run(cmd, env=dict(env, CVS_BENCH_TEST_CRASH_RANK="1"), capture_output=True, text=True, timeout=900)
    assert r.returncode != 0
    d = _json_line(r.stdout)
    # rank 0 learns of it either from the parent's SIGTERM or from its own collective failing (gloo notices a dead peer)
    assert d["n_gpus"] == 2 and d["value"] > 0 and ("SIGTERM" in d["extra_error"] or "secondary legs failed" in d["extra_error"])
