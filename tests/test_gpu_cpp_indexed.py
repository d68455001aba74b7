"""GPU: the C++ host mirror (include/mpjx.hpp) with Datatype::Indexed / Hindexed / Hvector on the block moves
(tests/cpp/indexed_tests.cpp): the mirror's bounds and exceptions, the reference's upper triangle packed and
unpacked, an Hvector of a Vector, and Alltoallv with an Indexed send type in multicore mode at P = 3 and 2."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_indexed_moves():
    exe = os.path.join(ROOT, "tests", "cpp", "indexed_tests")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mpjexpress_amd"), "tests"])
    r = subprocess.run([exe, "3", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "ALL INDEXED TESTS PASSED" in r.stdout and r.stdout.count("TEST COMPLETE") == 2, r.stdout
