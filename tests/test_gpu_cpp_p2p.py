"""GPU: the C++ host mirror (include/mpjx.hpp) running the reference's test/mpi/pt2pt/sendrecv.java and a 2 x 2
halo exchange (tests/cpp/p2p_tests.cpp) in multicore mode with one thread per rank, at P = 2, 3 and 4."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_point_to_point_programs():
    exe = os.path.join(ROOT, "tests", "cpp", "p2p_tests")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mpjexpress_amd"), "tests"])
    r = subprocess.run([exe, "2", "3", "4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "ALL P2P TESTS PASSED" in r.stdout and r.stdout.count("TEST COMPLETE") == 4, r.stdout
