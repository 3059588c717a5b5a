"""The steering bank (cvs_steer_bank) at every layer that exists without a GPU: the public header, the ctypes binding, the facade's
exports, the Python surface, and the generated code of its kernel instances."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "cvsteer_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def test_header_declares_steer_bank():
    text = open(os.path.join(ROOT, "include", "cvsteer_hip.h")).read()
    assert re.search(r"int cvs_steer_bank\(cvs_handle h, const float\* thetas, int n, const cvs_plane\* outs\);", text)
    assert re.search(r"#define CVS_ABI_VERSION 2\b", text)


def test_binding_has_steer_bank():
    import ctypes as C
    from cvsteer_amd import _lib as L
    res, args = L.SIGNATURES["cvs_steer_bank"]
    assert res is C.c_int
    assert args == [C.c_void_p, C.POINTER(C.c_float), C.c_int, C.POINTER(L.Plane)]
    fn = L.lib().cvs_steer_bank   # exported by the built library
    assert fn.argtypes == args


def test_bank_rejects_a_null_handle():
    import ctypes as C
    from cvsteer_amd import _lib as L
    th = (C.c_float * 2)(0.0, 1.0)
    planes = (L.Plane * 10)()
    assert L.lib().cvs_steer_bank(None, th, 2, planes) == L.E_BADARG


def test_facade_exports_vector_steer_overloads():
    so = os.path.join(ROOT, "cvsteer_amd", "libcvsteer.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cvsteer_amd", "facade"), "-s"])
    syms = subprocess.check_output(["nm", "-DC", "--defined-only", so], text=True)
    vf = "std::vector<float, std::allocator<float> > const&"
    vm = "std::vector<fa::Mat1f, std::allocator<fa::Mat1f> >&"
    for needle in ("fa::SteerableFiltersG2::steer(%s, %s, %s)" % (vf, vm, vm),
                   "fa::SteerableFiltersG2::steer(%s, %s, %s, %s, %s, %s)" % (vf, vm, vm, vm, vm, vm),
                   "fa::SteerableFiltersG4::steer(%s, %s, %s)" % (vf, vm, vm)):
        assert needle in syms, needle


def test_python_classes_have_steer_bank():
    import cvsteer_amd
    for cls in (cvsteer_amd.SteerableFiltersG2, cvsteer_amd.SteerableFiltersG4):
        assert callable(getattr(cls, "steer_bank", None)), cls


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_bank_instances_use_no_scratch(tmp_path):
    """every k_steer_bank instance (G2 / G4, float4 / dword) keeps its values in registers: no private segment"""
    path = os.path.join(str(tmp_path), "cvs_kernels_point.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    "-I" + SRC, "-S", "--cuda-device-only", os.path.join(SRC, "cvs_kernels_point.hip"), "-o", path], check=True, stderr=subprocess.DEVNULL)
    text = open(path).read()
    scratch = {}
    for blk in text.split("  - .agpr_count:")[1:]:
        nm = re.search(r"\.name:\s+(\S+)", blk)
        ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        if nm and ps:
            scratch[nm.group(1)] = int(ps.group(1))
    bank = {n: s for n, s in scratch.items() if "k_steer_bank" in n}
    assert len(bank) == 8, sorted(bank)
    assert {n for n in bank if "Li7E" in n} and {n for n in bank if "Li11E" in n}
    assert all(s == 0 for s in bank.values()), bank
