"""GPU: the C++ host mirror (include/mpjx.hpp) of Pack / Unpack / Pack_size (tests/cpp/pack_tests.cpp):
Pack_size's known values, two sections in one device image compared whole against bytes written by hand, an
Hindexed of DOUBLE with lb = 1 round trip, and Unpack of a section of another type or count throwing while the
array keeps its contents."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_pack_unpack():
    exe = os.path.join(ROOT, "tests", "cpp", "pack_tests")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mpjexpress_amd"), "tests"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "ALL PACK TESTS PASSED" in r.stdout, r.stdout
