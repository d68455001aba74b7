"""CPU: the ABI surface and the host-side planner of the reductions on derived datatypes (no GPU).

  - include/mpjx.h declares mpjx_reduce_dt, mpjx_allreduce_dt, mpjx_reduce_scatter_dt, mpjx_scan_dt and
    mpjx_comm_last_dt_form with their counterparts' arguments, libmpjx exports them and the ctypes table binds
    them.
  - The errors a call answers before it needs a communicator, through the C ABI with a NULL one: an unknown or
    freed type, a type whose own blocks share a byte, MPJX_ERR_OP_TYPE on the base type, MPJX_FLAG_FAITHFUL and
    the big-endian flags with a derived type; then the NULL communicator itself. (The errors of a whole world
    — mismatched ranks, a rank's overlapping layouts — need ranks: tests/test_gpu_reduce_dt.py.)
  - The existing entry points answer derived codes as before.
  - The mirror raises MPIException for a derived type on host arrays.
  - tests/cpp/reduce_dt_plan_test.cpp, a stand-alone program over mpjexpress_amd/csrc/mpjx_reduce_dt_plan.hpp,
    is compiled with plain g++ under AddressSanitizer and UBSan and run.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from test_strided_abi import build_and_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "mpjx.h")
NEW = ("mpjx_reduce_dt", "mpjx_allreduce_dt", "mpjx_reduce_scatter_dt", "mpjx_scan_dt", "mpjx_comm_last_dt_form")
ERR_ARG, ERR_OP_TYPE, ERR_UNSUPPORTED = -1, -2, -6
INT, DOUBLE, DOUBLE2 = 5, 8, 0x108
SUM, BAND, MAXLOC = 3, 6, 11
FAITHFUL, SEND_BE, RECV_BE = 0x2, 0x4, 0x8


@pytest.fixture(scope="module")
def L():
    from mpjexpress_amd import _lib

    return _lib.lib()


def vector(L, count, blocklength, stride, old):
    code = ctypes.c_int(-1)
    assert L.mpjx_type_vector(count, blocklength, stride, old, ctypes.byref(code)) == 0
    return code.value


def indexed(L, bl, disp, old):
    arr = ctypes.c_int64 * len(bl)
    code = ctypes.c_int(-1)
    assert L.mpjx_type_indexed(len(bl), arr(*bl), arr(*disp), old, ctypes.byref(code)) == 0
    return code.value


def all_four(L, type_, op, flags=0):
    """The four calls' answers to a NULL communicator and NULL buffers, and the last message"""
    rc1 = (ctypes.c_int64 * 1)(1)
    out = [L.mpjx_reduce_dt(None, None, None, 1, type_, op, 0, flags, None),
           L.mpjx_allreduce_dt(None, None, None, 1, type_, op, flags, None),
           L.mpjx_reduce_scatter_dt(None, None, None, rc1, type_, op, flags, None),
           L.mpjx_scan_dt(None, None, None, 1, type_, op, flags, None)]
    return out, L.mpjx_last_error()


def test_header_declares_the_five_functions():
    txt = open(HDR).read()
    fns = set(re.findall(r"^int\s+(mpjx_[a-z_]+)\(", txt, re.M))
    for f in NEW:
        assert f in fns, f

    def args(name):
        return " ".join(re.search(rf"int {name}\(([^;]*)\);", txt).group(1).split())
    for name in ("mpjx_reduce", "mpjx_allreduce", "mpjx_reduce_scatter", "mpjx_scan"):
        assert args(name + "_dt") == args(name), name  # the counterparts' arguments
    assert args("mpjx_comm_last_dt_form") == "mpjx_comm_t comm, int *form"
    forms = dict(re.findall(r"^#define (MPJX_DT_FORM_[A-Z]+) (\d+)", txt, re.M))
    assert forms == {"MPJX_DT_FORM_CONTIGUOUS": "1", "MPJX_DT_FORM_MOVE": "2", "MPJX_DT_FORM_DIRECT": "3",
                     "MPJX_DT_FORM_PACK": "4"}


def test_library_exports_and_binds_them(L):
    from mpjexpress_amd import _lib

    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for f in NEW:
        assert f in exported, f
        assert f in _lib.EXPORTS, f
        assert getattr(L, f).restype is ctypes.c_int
    for name in ("mpjx_reduce", "mpjx_allreduce", "mpjx_reduce_scatter", "mpjx_scan"):
        assert getattr(L, name + "_dt").argtypes == getattr(L, name).argtypes, name


def test_unknown_and_freed_types_are_err_arg(L):
    for bad in (0, 9, 0x104, 0x10000 + 10 ** 6):
        out, msg = all_four(L, bad, SUM)
        assert out == [ERR_ARG] * 4 and b"unknown or freed datatype code" in msg, (bad, out, msg)
    v = vector(L, 6, 2, 5, INT)
    assert L.mpjx_type_free(v) == 0
    out, msg = all_four(L, v, SUM)
    assert out == [ERR_ARG] * 4 and str(v).encode() in msg


def test_a_type_whose_blocks_share_a_byte_is_err_arg(L):
    t = indexed(L, [2, 2], [0, 1], INT)  # elements 0-1 and 1-2
    try:
        out, msg = all_four(L, t, SUM)
        assert out == [ERR_ARG] * 4 and b"share a byte" in msg and str(t).encode() in msg, (out, msg)
    finally:
        assert L.mpjx_type_free(t) == 0


def test_op_type_is_checked_on_the_base_type(L):
    vi, vd, vp = vector(L, 6, 2, 5, INT), vector(L, 6, 2, 5, DOUBLE), vector(L, 3, 2, 4, DOUBLE2)
    try:
        for type_, op, word in ((vi, MAXLOC, b"MAXLOC"), (vd, BAND, b"BAND"), (vp, SUM, b"DOUBLE2"), (vd, 5, b"LAND")):
            out, msg = all_four(L, type_, op)
            assert out == [ERR_OP_TYPE] * 4 and word in msg, (type_, op, out, msg)
        out, msg = all_four(L, vi, 99)
        assert out == [ERR_ARG] * 4 and b"unknown op code" in msg
        # valid pairs reach the communicator check: MAXLOC reduces a type made of pairs
        for type_, op in ((vi, SUM), (vi, BAND), (vd, SUM), (vp, MAXLOC)):
            out, msg = all_four(L, type_, op)
            assert out == [ERR_ARG] * 4 and b"comm is NULL" in msg, (type_, op, out, msg)
    finally:
        for t in (vi, vd, vp):
            assert L.mpjx_type_free(t) == 0


def test_faithful_and_big_endian_with_a_derived_type_are_unsupported(L):
    v = vector(L, 6, 2, 5, INT)
    try:
        out, msg = all_four(L, v, SUM, FAITHFUL)
        assert out == [ERR_UNSUPPORTED] * 4 and b"MPJX_FLAG_FAITHFUL" in msg and str(v).encode() in msg, (out, msg)
        for f in (SEND_BE, RECV_BE, SEND_BE | RECV_BE):
            out, msg = all_four(L, v, SUM, f)
            assert out == [ERR_UNSUPPORTED] * 4 and b"big-endian" in msg, (f, out, msg)
        # with a basic code the flags are the contiguous call's business: it asks for its communicator
        out, msg = all_four(L, INT, SUM, FAITHFUL | SEND_BE)
        assert out == [ERR_ARG] * 4 and (b"comm is NULL" in msg), (out, msg)
    finally:
        assert L.mpjx_type_free(v) == 0


def test_null_communicator_is_err_arg(L):
    f = ctypes.c_int(7)
    assert L.mpjx_comm_last_dt_form(None, ctypes.byref(f)) == ERR_ARG and f.value == 7
    assert b"comm is NULL" in L.mpjx_last_error()


def test_existing_entry_points_answer_derived_codes_as_before(L):
    v = vector(L, 6, 2, 5, INT)
    try:
        assert L.mpjx_type_size(v) == 0
        assert L.mpjx_op_check(SUM, v) == ERR_ARG
        rc1 = (ctypes.c_int64 * 1)(1)
        assert L.mpjx_allreduce(None, None, None, 1, v, SUM, 0, None) == ERR_ARG
        assert L.mpjx_reduce(None, None, None, 1, v, SUM, 0, 0, None) == ERR_ARG
        assert L.mpjx_scan(None, None, None, 1, v, SUM, 0, None) == ERR_ARG
        assert L.mpjx_reduce_scatter(None, None, None, rc1, v, SUM, 0, None) == ERR_ARG
    finally:
        assert L.mpjx_type_free(v) == 0


def test_the_mirror_refuses_a_derived_type_on_host_arrays():
    from mpjexpress_amd.mpi import MPI, Datatype, Intracomm, MPIException

    c = Intracomm.__new__(Intracomm)  # no communicator is needed to be refused
    c._h, c._rank, c._size, c.faithful, c.device = ctypes.c_void_p(None), 0, 1, False, 0
    v = Datatype.Vector(3, 2, 5, MPI.INT)
    a, b = np.zeros(64, np.int32), np.zeros(64, np.int32)
    try:
        for call in (lambda: c.Allreduce(a, 0, b, 0, 2, v, MPI.SUM), lambda: c.Reduce(a, 0, b, 0, 2, v, MPI.SUM, 0),
                     lambda: c.Scan(a, 0, b, 0, 2, v, MPI.SUM), lambda: c.Reduce_scatter(a, 0, b, 0, [2], v, MPI.SUM)):
            with pytest.raises(MPIException, match="device-resident"):
                call()
    finally:
        v.Free()


def test_planner_under_sanitizers(tmp_path):
    build_and_run(tmp_path, "reduce_dt_plan_test", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
