"""CPU tests (-m "not gpu") of the batch drivers' --g4 flag: both drivers accept it and list it in their usage line, and
the G2 defaults stay as they were."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_python_driver_lists_g4():
    r = subprocess.run([sys.executable, "-m", "cvsteer_amd.run", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--g4" in r.stdout and "--gain" in r.stdout and "--ext" in r.stdout


def test_cpp_driver_lists_g4():
    exe = os.path.join(ROOT, "cvsteer_amd", "cvsteer-run")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cvsteer_amd", "facade"), "-s"])
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == ("usage: cvsteer-run --input <image | list.txt> --output <dir> [--gain G] [--gpus N | --devices a,b,..] "
                                "[--ext .pgm|.npy] [--g4] [--verbose]")
