"""CPU: the ABI surface of Pack / Unpack / Pack_size and their host-side planner (no GPU).

  - include/mpjx.h declares mpjx_pack_size, mpjx_pack and mpjx_unpack, libmpjx exports them, the ctypes table
    binds them.
  - mpjx_pack_size returns the reference's values, padding quirk included (src/mpi/BasicType.java:209-220).
  - every MPJX_ERR_ARG case of mpjx_pack / mpjx_unpack is returned before the communicator is looked at, so with
    no device at all: each is reached with comm = NULL and told apart by its message. Pointers here are made-up
    addresses; a rejected call dereferences none of them.
  - tests/cpp/pack_plan_test.cpp (section arithmetic, the int32 limit, pack_size, header bytes, the granule, every
    granule's address) under AddressSanitizer and UBSan.
"""
import ctypes
import os
import re
import subprocess

import pytest

from test_strided_abi import build_and_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "mpjx.h")
NEW = ("mpjx_pack_size", "mpjx_pack", "mpjx_unpack")
MPJX_ERR_ARG = -1
BYTE, SHORT, INT, DOUBLE, FLOAT2 = 1, 3, 5, 8, 0x107
BUF, IMG, STATUS = 0x7F0000001000, 0x7F0000100000, 0x7F0000200000  # never dereferenced


@pytest.fixture(scope="module")
def L():
    from mpjexpress_amd import _lib

    return _lib.lib()


def arr(v):
    return (ctypes.c_int64 * max(len(v), 1))(*v)


def vector(L, count, bl, stride, old):
    code = ctypes.c_int(-1)
    assert L.mpjx_type_vector(count, bl, stride, old, ctypes.byref(code)) == 0
    return code.value


def pack(L, buf, count, type_, image, image_bytes, position, comm=None):
    pos = ctypes.c_int64(position)
    rc = L.mpjx_pack(comm, buf, count, type_, image, image_bytes, ctypes.byref(pos), None)
    return rc, pos.value, L.mpjx_last_error()


def unpack(L, image, image_bytes, position, buf, count, type_, status=STATUS, comm=None):
    pos = ctypes.c_int64(position)
    rc = L.mpjx_unpack(comm, image, image_bytes, ctypes.byref(pos), buf, count, type_, status, None)
    return rc, pos.value, L.mpjx_last_error()


def test_header_declares_the_three_functions():
    txt = open(HDR).read()
    for proto in (r"int mpjx_pack_size\(int64_t count, int type, int64_t \*bytes\);",
                  r"int mpjx_pack\(mpjx_comm_t comm, const void \*inbuf, int64_t count, int type, void \*image, "
                  r"int64_t image_bytes,\s+int64_t \*position, void \*stream\);",
                  r"int mpjx_unpack\(mpjx_comm_t comm, const void \*image, int64_t image_bytes, int64_t \*position, "
                  r"void \*outbuf,\s+int64_t count, int type, int \*status, void \*stream\);"):
        assert re.search(proto, txt), proto
    assert "upper bound" in txt and "t + t % 8" in txt


def test_library_exports_and_binds_them(L):
    from mpjexpress_amd import _lib

    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for f in NEW:
        assert f in exported and f in _lib.EXPORTS, f
        assert getattr(L, f).restype is ctypes.c_int


def test_pack_size_known_values(L):
    def size(count, type_):
        n = ctypes.c_int64(-1)
        assert L.mpjx_pack_size(count, type_, ctypes.byref(n)) == 0
        return n.value
    assert size(1, BYTE) == 10 and size(3, BYTE) == 14 and size(1, SHORT) == 12
    assert size(1, INT) == 16 and size(1, DOUBLE) == 16 and size(0, DOUBLE) == 8
    assert size(3, FLOAT2) == 32  # a pair is two base elements: t = 8 + 24
    v = vector(L, 3, 2, 5, INT)
    assert size(2, v) == 56
    assert L.mpjx_type_free(v) == 0
    n = ctypes.c_int64(-1)
    assert L.mpjx_pack_size(2, v, ctypes.byref(n)) == MPJX_ERR_ARG and b"freed" in L.mpjx_last_error()
    assert L.mpjx_pack_size(-1, INT, ctypes.byref(n)) == MPJX_ERR_ARG and b"negative count -1" in L.mpjx_last_error()
    assert L.mpjx_pack_size(1, INT, None) == MPJX_ERR_ARG
    assert L.mpjx_pack_size(1 << 61, DOUBLE, ctypes.byref(n)) == MPJX_ERR_ARG and b"2^62" in L.mpjx_last_error()
    assert n.value == -1


def test_a_good_call_reaches_the_communicator_check(L):
    """The yardstick for the cases below: with sound arguments the only complaint left is the NULL communicator."""
    rc, pos, msg = pack(L, BUF, 3, INT, IMG, 64, 5)
    assert rc == MPJX_ERR_ARG and b"comm is NULL" in msg and pos == 5
    rc, pos, msg = unpack(L, IMG, 64, 5, BUF, 3, INT)
    assert rc == MPJX_ERR_ARG and b"comm is NULL" in msg and pos == 5
    rc, _, msg = pack(L, None, 0, INT, IMG, 8, 0)  # count 0 needs no buffer
    assert rc == MPJX_ERR_ARG and b"comm is NULL" in msg
    rc, _, msg = pack(L, BUF, 3, INT, IMG, 28, 5)  # header at 8, 12 payload bytes: exactly 28
    assert rc == MPJX_ERR_ARG and b"comm is NULL" in msg


def each(L, what, *words, **kw):
    """The same rejected arguments through mpjx_pack and mpjx_unpack."""
    buf, count, type_, image, nbytes, position = what
    for rc, pos, msg in (pack(L, buf, count, type_, image, nbytes, position),
                         unpack(L, image, nbytes, position, buf, count, type_, **kw)):
        assert rc == MPJX_ERR_ARG and pos == position, (rc, pos, msg)
        assert b"comm is NULL" not in msg, msg
        for w in words:
            assert w in msg, (w, msg)


def test_err_arg_cases_need_no_device(L):
    each(L, (None, 3, INT, IMG, 64, 0), b"NULL", b"count 3")
    each(L, (BUF, 3, INT, None, 64, 0), b"image is NULL")
    each(L, (BUF, -1, INT, IMG, 64, 0), b"negative count -1")
    each(L, (BUF, 1, INT, IMG, 64, -8), b"negative position -8")
    each(L, (BUF, 1 << 31, BYTE, IMG, 1 << 40, 0), b"int32")       # count * Size() above 2^31 - 1
    each(L, (BUF, 1 << 30, FLOAT2, IMG, 1 << 40, 0), b"int32")      # 2^31 base elements
    each(L, (BUF + 2, 3, INT, IMG, 64, 0), b"not aligned", b"4-byte")
    each(L, (BUF + 4, 3, DOUBLE, IMG, 64, 0), b"not aligned", b"8-byte")
    each(L, (BUF + 1, 3, SHORT, IMG, 64, 0), b"not aligned", b"2-byte")
    each(L, (BUF, 3, INT, IMG + 4, 64, 0), b"8-byte aligned")
    each(L, (BUF, 3, INT, IMG, 27, 5), b"ends past the image", b"27")  # one byte short of 8 + 8 + 12
    each(L, (BUF, 0, INT, IMG, 15, 5), b"ends past the image")          # the header alone does not fit
    each(L, (BUF, 3, INT, IMG, 64, 65), b"ends past the image")
    each(L, (BUF, 3, 0x101, IMG, 64, 0), b"unknown or freed datatype code 257")
    # NULL position and (unpack) NULL status
    assert L.mpjx_pack(None, BUF, 1, INT, IMG, 64, None, None) == MPJX_ERR_ARG and b"position is NULL" in L.mpjx_last_error()
    rc, _, msg = unpack(L, IMG, 64, 0, BUF, 1, INT, status=None)
    assert rc == MPJX_ERR_ARG and b"status is NULL" in msg
    # BYTE buffers sit at any address
    rc, _, msg = pack(L, BUF + 3, 5, BYTE, IMG, 64, 0)
    assert b"comm is NULL" in msg


def test_unpack_rejects_a_self_overlapping_type(L):
    code = ctypes.c_int(-1)
    assert L.mpjx_type_indexed(2, arr([3, 3]), arr([0, 2]), INT, ctypes.byref(code)) == 0  # [0,3) and [2,5)
    rc, _, msg = unpack(L, IMG, 64, 0, BUF, 1, code.value)
    assert rc == MPJX_ERR_ARG and b"share a byte" in msg
    rc, _, msg = pack(L, BUF, 1, code.value, IMG, 64, 0)  # legal to pack
    assert rc == MPJX_ERR_ARG and b"comm is NULL" in msg
    assert L.mpjx_type_free(code.value) == 0
    each(L, (BUF, 1, code.value, IMG, 64, 0), b"unknown or freed datatype code")


def test_planner_under_sanitizers(tmp_path):
    build_and_run(tmp_path, "pack_plan_test", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
