"""CPU tests (no GPU) of the 8-bit pipeline outputs: the ABI surface (cvs_set_u8_gain / cvs_get_u8_gain, cvs_launch_info.u8_out) and
the new three-maps instances of the strip kernel in the gfx950 code object (present, byte stores in gain mode, no scratch)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from cvsteer_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "cvsteer_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
# FLAGS of the instances: F_ORIENT | F_PIPE | F_NOSTATE | F_FEAT3 and F_U8G (gain) or F_U8N (normalise)
GAIN_FLAGS, NORM_FLAGS = 1 | 4 | 8 | 64 | 128, 1 | 4 | 8 | 64 | 256


def test_library_exports_gain_functions():
    lib = C.CDLL(L.lib_path())
    for name in ("cvs_set_u8_gain", "cvs_get_u8_gain"):
        assert hasattr(lib, name)
        assert name in L.SIGNATURES


def test_launch_info_ends_with_u8_out():
    names = [n for n, _ in L.LaunchInfo._fields_]
    assert names[-1] == "u8_out" and names[-2] == "literal_taps"
    assert C.sizeof(L.LaunchInfo) == 4 * 12   # 11 fields before, 4 bytes longer


def test_header_declares_gain_functions():
    text = open(os.path.join(ROOT, "include", "cvsteer_hip.h")).read()
    assert re.search(r"int cvs_set_u8_gain\(cvs_handle h, float gain\);", text)
    assert re.search(r"int cvs_get_u8_gain\(cvs_handle h, float\* gain\);", text)
    assert re.search(r"int32_t u8_out;", text)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_u8_instances_in_code_object(tmp_path):
    path = os.path.join(str(tmp_path), "cvs_kernels_basis.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-I" + os.path.join(ROOT, "include"),
                    "-I" + SRC, "-S", "--cuda-device-only", os.path.join(SRC, "cvs_kernels_basis.hip"), "-o", path], check=True, stderr=subprocess.DEVNULL)
    text = open(path).read()
    bodies = dict(re.findall(r"^(_ZN3cvs\w+):[^\n]*\n(.*?)s_endpgm", text, re.S | re.M))
    scratch = {}
    for blk in text.split("  - .agpr_count:")[1:]:
        nm = re.search(r"\.name:\s+(\S+)", blk)
        ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        if nm and ps:
            scratch[nm.group(1)] = int(ps.group(1))
    for flags, byte_stores in ((GAIN_FLAGS, True), (NORM_FLAGS, False)):
        names = [n for n in bodies if "Li%dE" % flags in n]
        lit = [n for n in names if "k_basis_lit" in n]
        assert len(names) >= 8 and lit, (flags, names)
        for n in names:
            assert scratch.get(n) == 0, (n, scratch.get(n))
            has_byte = "buffer_store_byte" in bodies[n]
            assert has_byte == byte_stores, n
