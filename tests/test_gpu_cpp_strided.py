"""GPU: the C++ host mirror (include/mpjx.hpp) with Datatype::Vector on the strided block moves
(tests/cpp/strided_tests.cpp): packed lengths around one and two tiles of the strided kernel, one call past its
streaming threshold, and Alltoallv / Gatherv with a Vector in multicore mode at P = 3 and 2."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_strided_moves():
    exe = os.path.join(ROOT, "tests", "cpp", "strided_tests")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mpjexpress_amd"), "tests"])
    r = subprocess.run([exe, "3", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "ALL STRIDED TESTS PASSED" in r.stdout and r.stdout.count("TEST COMPLETE") == 2, r.stdout
