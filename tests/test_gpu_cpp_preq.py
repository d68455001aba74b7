"""GPU: the C++ host mirror (include/mpjx.hpp) running persistent requests from C++ rank threads
(tests/cpp/preq_tests.cpp): reuse at P = 2, the 2 x 2 halo with the requests made once, and the pool's launch counts
for 30 and for 513 pairs waited on by one rank."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_persistent_request_programs():
    exe = os.path.join(ROOT, "tests", "cpp", "preq_tests")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mpjexpress_amd"), "tests"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "ALL PREQ TESTS PASSED" in r.stdout and r.stdout.count("TEST COMPLETE") == 4, r.stdout
