"""GPU: the C++ host mirror (include/mpjx.hpp) running the reference's block-move ccl programs
(test/mpi/ccl/{allgather,allgatherv,gatherv,scatterv,alltoall,alltoallv}.java, tests/cpp/moves_tests.cpp) in
multicore mode at P = 4 (and at the tables' own 3 tasks), against the `ans` tables kept as data in
tests/golden/ccl_moves_kat.json."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_block_move_known_answer_tests(tmp_path):
    exe = os.path.join(ROOT, "tests", "cpp", "moves_tests")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mpjexpress_amd"), "tests"])
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "ccl_moves_kat.json")))
    ans = tmp_path / "ans.txt"
    ans.write_text("\n".join(" ".join(str(v) for v in kat[k]["ans"]) for k in ("alltoallv", "allgatherv", "gatherv")))
    r = subprocess.run([exe, str(ans), "4", "3"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "ALL MOVES TESTS PASSED" in r.stdout and r.stdout.count("TEST COMPLETE") == 2, r.stdout
