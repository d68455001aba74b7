"""CPU: the ABI surface of MPI.PACKED messages, Probe and Iprobe, the mailbox's probe side and k_wire's planner
(no GPU).

  - include/mpjx.h declares the four prototypes verbatim and MPJX_PACKED = 9, libmpjx exports them, the ctypes table
    binds them (the three without a digit in EXPORTS), and each answers a NULL communicator or a bad argument with
    MPJX_ERR_ARG before touching anything.
  - mpjx_wire_bytes and mpjx_get_count(..., MPJX_PACKED) on hand-made statuses; PACKED stays unknown to every call
    that is not point-to-point.
  - tests/cpp/wire_plan_test.cpp (every lane of both directions of k_wire against a byte-wise model, table planning)
    under AddressSanitizer and UBSan; tests/cpp/p2p_probe_test.cpp (peek, probe, check; 8 threads) under ASan + UBSan
    and under ThreadSanitizer where that links and starts.
"""
import ctypes
import os
import re
import subprocess

import pytest

from test_p2p_abi import ASAN, build_and_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "mpjx.h")
MPJX_ERR_ARG, MPJX_UNDEFINED, MPJX_PACKED = -1, -1, 9
INT, BYTE = 5, 1

PROTOTYPES = """
int mpjx_iprobe(mpjx_comm_t comm, int source, int tag, int *flag, mpjx_status *status);
int mpjx_probe(mpjx_comm_t comm, int source, int tag, mpjx_status *status);
int mpjx_wire_bytes(const mpjx_status *status, int64_t *bytes);
int mpjx_comm_p2p_wire_stats(mpjx_comm_t comm, int64_t *launches, int64_t *packed, int64_t *unpacked,
                             int *table_max);
"""
NEW = re.findall(r"^int (mpjx_[a-z0-9_]+)\(", PROTOTYPES, re.M)


@pytest.fixture(scope="module")
def L():
    from mpjexpress_amd import _lib

    return _lib.lib()


def test_header_declares_every_prototype_verbatim():
    assert len(NEW) == 4
    txt = open(HDR).read()
    assert PROTOTYPES.strip() in txt
    assert re.search(r"\bMPJX_PACKED = 9\b", txt)
    # the new block comes after the existing ones
    assert txt.index("int mpjx_iprobe(") > txt.index("int mpjx_comm_p2p_pool_stats(")
    assert "Probe / Iprobe,\n * Bsend" not in txt  # no longer listed under "Not provided"


def test_library_exports_and_binds_them(L):
    from mpjexpress_amd import _lib

    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for f in NEW:
        assert f in exported, f
        assert f in _lib.BOUND, f
        assert getattr(L, f).restype is ctypes.c_int and getattr(L, f).argtypes is not None, f
    for f in ("mpjx_iprobe", "mpjx_probe", "mpjx_wire_bytes"):
        assert f in _lib.EXPORTS, f


def test_null_communicator_and_bad_arguments_are_err_arg(L):
    from mpjexpress_amd import _lib

    st, flag = _lib.Status(), ctypes.c_int(7)
    assert L.mpjx_iprobe(None, 0, 0, ctypes.byref(flag), ctypes.byref(st)) == MPJX_ERR_ARG
    assert b"comm is NULL" in L.mpjx_last_error() and flag.value == 0
    assert L.mpjx_probe(None, 0, 0, ctypes.byref(st)) == MPJX_ERR_ARG and b"comm is NULL" in L.mpjx_last_error()
    assert L.mpjx_comm_p2p_wire_stats(None, None, None, None, None) == MPJX_ERR_ARG
    # judged from the arguments alone, whatever the communicator is
    assert L.mpjx_iprobe(None, 0, 0, None, ctypes.byref(st)) == MPJX_ERR_ARG and b"flag is NULL" in L.mpjx_last_error()
    assert L.mpjx_iprobe(None, 0, -5, ctypes.byref(flag), None) == MPJX_ERR_ARG and b"tag -5" in L.mpjx_last_error()
    assert L.mpjx_probe(None, 0, -5, None) == MPJX_ERR_ARG and b"tag -5" in L.mpjx_last_error()
    assert L.mpjx_wire_bytes(None, None) == MPJX_ERR_ARG
    n = ctypes.c_int64()
    assert L.mpjx_wire_bytes(None, ctypes.byref(n)) == MPJX_ERR_ARG
    assert L.mpjx_wire_bytes(ctypes.byref(st), None) == MPJX_ERR_ARG
    # a PACKED request with a misaligned image or a NULL communicator
    h = ctypes.c_void_p()
    assert L.mpjx_isend(None, None, 0, MPJX_PACKED, 0, 0, ctypes.byref(h)) == MPJX_ERR_ARG
    assert L.mpjx_recv_init(None, None, 0, MPJX_PACKED, 0, 0, ctypes.byref(h)) == MPJX_ERR_ARG


def wire_bytes(L, elements, nbytes):
    from mpjexpress_amd import _lib

    st, n = _lib.Status(1, 7, 0, elements, nbytes), ctypes.c_int64(-99)
    return L.mpjx_wire_bytes(ctypes.byref(st), ctypes.byref(n)), n.value


def get_count(L, elements, code):
    from mpjexpress_amd import _lib

    st = _lib.Status(1, 7, 0, elements, 0)
    c, e = ctypes.c_int64(-99), ctypes.c_int64(-99)
    return L.mpjx_get_count(ctypes.byref(st), code, ctypes.byref(c), ctypes.byref(e)), c.value, e.value


def test_status_arithmetic(L):
    # a typed message needs its header; a PACKED one (elements unknown to the host) is an image already
    assert wire_bytes(L, 10, 40) == (0, 48)
    assert wire_bytes(L, 0, 0) == (0, 8)
    assert wire_bytes(L, MPJX_UNDEFINED, 72) == (0, 72)
    assert wire_bytes(L, MPJX_UNDEFINED, 0) == (0, 0)
    assert wire_bytes(L, 1, -4)[0] == MPJX_ERR_ARG
    # MPJX_PACKED counts bytes: size 1
    assert get_count(L, 48, MPJX_PACKED) == (0, 48, 48)
    assert get_count(L, 0, MPJX_PACKED) == (0, 0, 0)
    assert get_count(L, 48, BYTE) == (0, 48, 48) and get_count(L, 12, INT) == (0, 12, 12)


def test_packed_stays_unknown_outside_point_to_point(L):
    assert L.mpjx_type_size(MPJX_PACKED) == 0
    n = ctypes.c_int64()
    assert L.mpjx_pack_size(1, MPJX_PACKED, ctypes.byref(n)) == MPJX_ERR_ARG
    pos = ctypes.c_int64(0)
    assert L.mpjx_pack(None, None, 0, MPJX_PACKED, None, 8, ctypes.byref(pos), None) == MPJX_ERR_ARG
    assert b"datatype code 9" in L.mpjx_last_error()
    t = ctypes.c_int(-1)
    assert L.mpjx_type_contiguous(2, MPJX_PACKED, ctypes.byref(t)) == MPJX_ERR_ARG
    assert L.mpjx_type_vector(2, 1, 2, MPJX_PACKED, ctypes.byref(t)) == MPJX_ERR_ARG
    assert L.mpjx_op_check(3, MPJX_PACKED) != 0


def test_python_mirror_surface():
    from mpjexpress_amd import _lib
    from mpjexpress_amd.mpi import MPI, Intracomm, Status

    assert MPI.PACKED.code == 9 and MPI.PACKED.baseSize == 1
    for m in ("Probe", "Iprobe", "p2p_wire_stats"):
        assert callable(getattr(Intracomm, m)), m
    st = Status(_lib.Status(2, 9, 0, 10, 40))
    assert st.wire_bytes() == 48 and st.Get_count(MPI.PACKED) == 10
    assert Status(_lib.Status(2, 9, 0, MPI.UNDEFINED, 72)).wire_bytes() == 72


def test_wire_planner_under_asan_and_ubsan(tmp_path):
    build_and_run(tmp_path, "wire_plan_test", ASAN)


def test_probe_and_matching_under_asan_and_ubsan(tmp_path):
    build_and_run(tmp_path, "p2p_probe_test", ASAN, extra=("-pthread",))


def test_probe_and_matching_under_tsan(tmp_path):
    build_and_run(tmp_path, "p2p_probe_test", ["-fsanitize=thread"], extra=("-pthread",))
