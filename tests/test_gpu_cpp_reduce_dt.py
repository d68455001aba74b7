"""GPU: the C++ host mirror (include/mpjx.hpp) with Datatype::Vector on the reductions
(tests/cpp/reduce_dt_tests.cpp): Allreduce, Scan and Reduce_scatter at P = 4 rank threads on one device, each
through the layout-direct kernel, whole receive arrays compared; a derived type on host vectors throws."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_reductions_on_a_vector():
    exe = os.path.join(ROOT, "tests", "cpp", "reduce_dt_tests")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mpjexpress_amd"), "tests"])
    r = subprocess.run([exe, "4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "ALL REDUCE_DT TESTS PASSED" in r.stdout and r.stdout.count("TEST COMPLETE") == 1, r.stdout
