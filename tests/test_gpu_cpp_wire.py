"""GPU: the C++ host mirror (include/mpjx.hpp) running MPI.PACKED messages, Probe and Iprobe from C++ rank threads
(tests/cpp/wire_tests.cpp): several sections in one message, and probe -> wire_bytes -> Recv(PACKED) -> Unpack."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_wire_programs():
    exe = os.path.join(ROOT, "tests", "cpp", "wire_tests")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mpjexpress_amd"), "tests"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "ALL WIRE TESTS PASSED" in r.stdout and r.stdout.count("TEST COMPLETE") == 2, r.stdout
