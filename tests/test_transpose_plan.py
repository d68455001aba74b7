"""CPU: k_transpose's eligibility test and tile geometry, and the planner's handling of explicit bounds.

tests/cpp/transpose_plan_test.cpp is a stand-alone program over mpjexpress_amd/csrc/mpjx_transpose_plan.hpp, the
header the kernel itself includes; it is built and run here under AddressSanitizer and UBSan, like the other plan
tests. The Makefile builds it too (plain g++), next to them.
"""
import os

from test_strided_abi import build_and_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_transpose_planner_under_sanitizers(tmp_path):
    build_and_run(tmp_path, "transpose_plan_test", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_the_kernel_includes_the_header_the_test_walks():
    k = open(os.path.join(ROOT, "mpjexpress_amd", "csrc", "mpjx_k_transpose.hip")).read()
    assert '#include "mpjx_transpose_plan.hpp"' in k
    for fn in ("tr_slot(", "tr_addr_x(", "tr_addr_y(", "tr_lds("):
        assert fn in k, fn
    assert "asm" not in k  # plain C++: no inline assembly
