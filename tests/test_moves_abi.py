"""CPU: the block-move collectives' ABI surface and host-side planner (no GPU).

  - include/mpjx.h declares mpjx_allgather, mpjx_allgatherv, mpjx_gatherv, mpjx_scatterv, mpjx_alltoall and
    mpjx_alltoallv, libmpjx exports them, the ctypes table binds them, and each answers a NULL communicator
    with MPJX_ERR_ARG before touching anything.
  - tests/cpp/moves_plan_test.cpp, a stand-alone program over mpjexpress_amd/csrc/mpjx_moves_plan.hpp, is
    compiled with plain g++ under AddressSanitizer and UBSan and run: tile coverage for P in {1, 3, 8, 9, 64},
    every alignment pair, rejections, 2^31 + 5 doubles, alltoallv.java's shape.
"""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "mpjx.h")
MOVES = ("mpjx_allgather", "mpjx_allgatherv", "mpjx_gatherv", "mpjx_scatterv", "mpjx_alltoall", "mpjx_alltoallv")
MPJX_ERR_ARG = -1


def test_header_declares_the_six_block_moves():
    txt = open(HDR).read()
    fns = set(re.findall(r"^int\s+(mpjx_[a-z_]+)\(", txt, re.M))
    for f in MOVES:
        assert f in fns, f
    # counts and displacements are 64-bit element counts; no flags argument
    m = re.search(r"int mpjx_alltoallv\(([^;]*)\);", txt)
    args = " ".join(m.group(1).split())
    assert args == ("mpjx_comm_t comm, const void *sendbuf, const int64_t *sendcounts, const int64_t *sdispls, "
                    "void *recvbuf, const int64_t *recvcounts, const int64_t *rdispls, int type, void *stream")


def test_library_exports_and_binds_them():
    from mpjexpress_amd import _lib

    L = _lib.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for f in MOVES:
        assert f in exported, f
        assert f in _lib.EXPORTS, f
        assert getattr(L, f).restype is ctypes.c_int


def test_null_communicator_is_err_arg():
    from mpjexpress_amd import _lib

    L = _lib.lib()
    tab = (ctypes.c_int64 * 1)(0)
    assert L.mpjx_allgather(None, None, None, 0, 5, None) == MPJX_ERR_ARG
    assert L.mpjx_allgatherv(None, None, 0, None, tab, tab, 5, None) == MPJX_ERR_ARG
    assert L.mpjx_gatherv(None, None, 0, None, tab, tab, 5, 0, None) == MPJX_ERR_ARG
    assert L.mpjx_scatterv(None, None, tab, tab, None, 0, 5, 0, None) == MPJX_ERR_ARG
    assert L.mpjx_alltoall(None, None, None, 0, 5, None) == MPJX_ERR_ARG
    assert L.mpjx_alltoallv(None, None, tab, tab, None, tab, tab, 5, None) == MPJX_ERR_ARG
    assert b"comm is NULL" in L.mpjx_last_error()


def test_python_mirror_has_the_mpijava_methods():
    from mpjexpress_amd import mpi

    for name in ("Allgather", "Allgatherv", "Gatherv", "Scatterv", "Alltoall", "Alltoallv"):
        assert callable(getattr(mpi.Intracomm, name)), name


def test_planner_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/cpp/moves_plan_test.cpp"
    src = os.path.join(ROOT, "tests", "cpp", "moves_plan_test.cpp")
    exe = str(tmp_path / "moves_plan_test")
    base = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", src, "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True,
                       text=True)
    if r.returncode != 0 and re.search(r"cannot find|libasan|libubsan", r.stderr):
        print("sanitizer runtimes absent: built without them\n" + r.stderr[-500:])
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "moves_plan_test: ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
