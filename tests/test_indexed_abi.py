"""CPU: the irregular datatypes' ABI surface, forms and host-side planner (no GPU).

  - include/mpjx.h declares mpjx_type_hvector, mpjx_type_indexed, mpjx_type_hindexed and mpjx_type_layout,
    libmpjx exports them, the ctypes table binds them; a NULL newtype is MPJX_ERR_ARG.
  - the forms through mpjx_type_info / mpjx_type_layout: the reference's cases (test/mpi/dtyp/Indexed.java,
    hvec.java), merging, normalisation to the regular form, empty types; every error with a message that names
    what was passed; use after free; the older entry points keep rejecting the new codes.
  - tests/cpp/indexed_plan_test.cpp (forms, the address function of k_indexed against a walk of the block list,
    granule, launch tables, overlap) under AddressSanitizer and UBSan; tests/cpp/indexed_registry_test.cpp
    (threads creating and freeing the new types) under ThreadSanitizer where that links and starts.
  - the Python mirror's Size / Extent / Lb / Ub and exceptions.
"""
import ctypes
import os
import re
import subprocess

import pytest

from test_strided_abi import build_and_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "mpjx.h")
NEW = ("mpjx_type_hvector", "mpjx_type_indexed", "mpjx_type_hindexed", "mpjx_type_layout")
MPJX_ERR_ARG, MPJX_ERR_UNSUPPORTED = -1, -6
BYTE, INT, DOUBLE, DOUBLE2 = 1, 5, 8, 0x108


@pytest.fixture(scope="module")
def L():
    from mpjexpress_amd import _lib

    return _lib.lib()


def arr(v):
    return (ctypes.c_int64 * max(len(v), 1))(*v)


def layout(L, code):
    """(base, size, extent, lb, ub, merged blocks, regular) of a live code."""
    base, size, extent = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()
    lb, ub, nb, reg = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int(-1)
    assert L.mpjx_type_info(code, ctypes.byref(base), ctypes.byref(size), ctypes.byref(extent)) == 0
    assert L.mpjx_type_layout(code, ctypes.byref(lb), ctypes.byref(ub), ctypes.byref(nb), ctypes.byref(reg)) == 0
    return base.value, size.value, extent.value, lb.value, ub.value, nb.value, reg.value


def indexed(L, bl, disp, old, fn="mpjx_type_indexed"):
    code = ctypes.c_int(-1)
    return getattr(L, fn)(len(bl), arr(bl), arr(disp), old, ctypes.byref(code)), code.value


def hindexed(L, bl, disp, old):
    return indexed(L, bl, disp, old, "mpjx_type_hindexed")


def hvector(L, count, bl, stride, old):
    code = ctypes.c_int(-1)
    return L.mpjx_type_hvector(count, bl, stride, old, ctypes.byref(code)), code.value


def made(r):
    assert r[0] == 0 and r[1] >= 0x10000, r
    return r[1]


def test_header_declares_the_four_functions():
    txt = open(HDR).read()
    for proto in (r"int mpjx_type_hvector\(int64_t count, int64_t blocklength, int64_t stride, int oldtype, int \*newtype\);",
                  r"int mpjx_type_indexed\(int n, const int64_t \*blocklengths, const int64_t \*displacements, int oldtype, "
                  r"int \*newtype\);",
                  r"int mpjx_type_hindexed\(int n, const int64_t \*blocklengths, const int64_t \*displacements, int oldtype, "
                  r"int \*newtype\);",
                  r"int mpjx_type_layout\(int type, int64_t \*lb, int64_t \*ub, int64_t \*nblocks, int \*regular\);"):
        assert re.search(proto, txt), proto
    assert "1,048,576 blocks" in txt and "supported spelling of a Vector of a" in txt


def test_library_exports_and_binds_them(L):
    from mpjexpress_amd import _lib

    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for f in NEW:
        assert f in exported and f in _lib.EXPORTS, f
        assert getattr(L, f).restype is ctypes.c_int
    assert L.mpjx_type_hvector(2, 1, 2, INT, None) == MPJX_ERR_ARG
    assert L.mpjx_type_indexed(1, arr([1]), arr([0]), INT, None) == MPJX_ERR_ARG
    assert L.mpjx_type_hindexed(1, arr([1]), arr([0]), INT, None) == MPJX_ERR_ARG
    assert L.mpjx_type_layout(INT, None, None, None, None) == 0  # every out pointer is optional


def test_layout_of_the_existing_types(L):
    assert layout(L, INT) == (INT, 1, 1, 0, 1, 1, 1)
    assert layout(L, DOUBLE2) == (DOUBLE, 2, 2, 0, 2, 1, 1)
    v = ctypes.c_int()
    assert L.mpjx_type_vector(6, 2, 5, INT, ctypes.byref(v)) == 0
    assert layout(L, v.value) == (INT, 12, 27, 0, 27, 6, 1)
    assert L.mpjx_type_free(v.value) == 0
    assert L.mpjx_type_layout(v.value, None, None, None, None) == MPJX_ERR_ARG
    assert L.mpjx_type_layout(0, None, None, None, None) == MPJX_ERR_ARG


def test_indexed_forms(L):
    t = []
    t.append(made(indexed(L, [3, 1, 0, 2], [7, 0, 4, 12], INT)))
    assert layout(L, t[-1]) == (INT, 6, 14, 0, 14, 3, 0)  # the empty block dropped
    t.append(made(indexed(L, [2, 1], [9, 4], INT)))
    assert layout(L, t[-1]) == (INT, 3, 7, 4, 11, 2, 0)  # lb 4, ub 11
    # over DOUBLE2 Indexed counts in pairs; Hindexed takes the same offsets in base elements
    t.append(made(indexed(L, [2, 1], [9, 4], DOUBLE2)))
    t.append(made(hindexed(L, [2, 1], [18, 8], DOUBLE2)))
    assert layout(L, t[-2]) == layout(L, t[-1]) == (DOUBLE, 6, 14, 8, 22, 2, 0)
    t.append(made(hindexed(L, [2, 1], [9, 4], DOUBLE2)))  # offsets as given: 9 and 4 doubles
    assert layout(L, t[-1]) == (DOUBLE, 6, 9, 4, 13, 2, 0)
    # the reference's triangle: row i of an 8 x 8 matrix from its diagonal on
    t.append(made(indexed(L, [8 - i for i in range(8)], [9 * i for i in range(8)], DOUBLE)))
    assert layout(L, t[-1]) == (DOUBLE, 36, 64, 0, 64, 8, 0)
    # abutting blocks merge (in pack order and address order only)
    t.append(made(indexed(L, [2, 3, 1], [0, 2, 9], INT)))
    assert layout(L, t[-1]) == (INT, 6, 10, 0, 10, 2, 0)
    t.append(made(indexed(L, [2, 2], [2, 0], INT)))
    assert layout(L, t[-1]) == (INT, 4, 4, 0, 4, 2, 0)
    # equal blocks at a constant stride ARE the Vector
    t.append(made(indexed(L, [2] * 6, [5 * i for i in range(6)], INT)))
    assert layout(L, t[-1]) == (INT, 12, 27, 0, 27, 6, 1)
    t.append(made(indexed(L, [2, 2], [0, 2], INT)))
    assert layout(L, t[-1]) == (INT, 4, 4, 0, 4, 1, 1)
    # Indexed([2],[3],INT): lb 3, extent 2
    t.append(made(indexed(L, [2], [3], INT)))
    assert layout(L, t[-1]) == (INT, 2, 2, 3, 5, 1, 0)
    for code in t:
        assert L.mpjx_type_size(code) == 0
        assert L.mpjx_type_free(code) == 0


def test_hvector_of_a_vector(L):
    """The shapes of test/mpi/dtyp/hvec.java: Hvector(3, 1, ext + off, Vector(2, 3, 4, INT)), ext = 7."""
    v = ctypes.c_int()
    assert L.mpjx_type_vector(2, 3, 4, INT, ctypes.byref(v)) == 0
    want = {0: (INT, 18, 21, 0, 21, 4, 0),   # [4,7) and [7,10) abut: 4 blocks
            1: (INT, 18, 23, 0, 23, 6, 1),   # 6 blocks of 3 every 4: Vector(6, 3, 4, INT)
            2: (INT, 18, 25, 0, 25, 6, 0),
            -1: (INT, 18, 19, 0, 19, 6, 0)}  # constructs; its blocks [4,7) and [6,9) share an element
    for off, exp in want.items():
        h = made(hvector(L, 3, 1, 7 + off, v.value))
        assert layout(L, h) == exp, off
        assert L.mpjx_type_free(h) == 0
    # the Vector entry points still refuse a non-contiguous oldtype; Hvector is the spelling
    vv = ctypes.c_int(-1)
    assert L.mpjx_type_vector(2, 1, 2, v.value, ctypes.byref(vv)) == MPJX_ERR_UNSUPPORTED
    h = made(hvector(L, 2, 1, 2 * 7, v.value))
    assert layout(L, h) == (INT, 12, 21, 0, 21, 4, 0)  # Vector(2, 1, 2, v): blocks at 0, 4, 14, 18
    irr = made(indexed(L, [2, 1], [9, 4], INT))
    assert L.mpjx_type_vector(2, 1, 2, irr, ctypes.byref(vv)) == MPJX_ERR_UNSUPPORTED
    assert b"irregular oldtype" in L.mpjx_last_error()
    assert L.mpjx_type_contiguous(2, irr, ctypes.byref(vv)) == MPJX_ERR_UNSUPPORTED
    nest = made(indexed(L, [2, 1], [0, 3], irr))  # an irregular oldtype is flattened: 3 items, 2 blocks each
    assert layout(L, nest) == (INT, 9, 28, 4, 32, 6, 0)
    for code in (h, irr, nest, v.value):
        assert L.mpjx_type_free(code) == 0


def test_empty_types(L):
    for r in (indexed(L, [], [], INT), indexed(L, [0, 0], [5, 9], INT), hindexed(L, [0], [-3], DOUBLE2),
              hvector(L, 0, 3, 2, INT), hvector(L, 4, 0, 2, INT), hvector(L, 1, 0, -9, INT)):
        code = made(r)
        assert layout(L, code)[1:5] == (0, 0, 0, 0)
        assert L.mpjx_type_free(code) == 0


def test_errors_name_what_was_passed(L):
    def err(r, status, *words):
        assert r[0] == status and r[1] == -1, r
        msg = L.mpjx_last_error()
        for w in words:
            assert w in msg, (w, msg)
    err(indexed(L, [2, -7], [0, 4], INT), MPJX_ERR_ARG, b"Indexed", b"-7", b"index 1")
    err(hindexed(L, [-2], [0], INT), MPJX_ERR_ARG, b"Hindexed", b"-2")
    err(hvector(L, -3, 1, 2, INT), MPJX_ERR_ARG, b"Hvector", b"count -3")
    err(hvector(L, 2, -5, 2, INT), MPJX_ERR_ARG, b"blocklength -5")
    code = ctypes.c_int(-1)
    assert L.mpjx_type_indexed(-4, arr([1]), arr([0]), INT, ctypes.byref(code)) == MPJX_ERR_ARG
    assert b"n -4" in L.mpjx_last_error()
    assert L.mpjx_type_indexed(2, None, arr([0, 1]), INT, ctypes.byref(code)) == MPJX_ERR_ARG
    assert b"NULL blocklengths" in L.mpjx_last_error() and b"n = 2" in L.mpjx_last_error()
    assert L.mpjx_type_hindexed(2, arr([1, 1]), None, INT, ctypes.byref(code)) == MPJX_ERR_ARG
    assert b"NULL displacements" in L.mpjx_last_error()
    assert L.mpjx_type_indexed(0, None, None, INT, ctypes.byref(code)) == 0  # no arrays needed for none
    assert L.mpjx_type_free(code.value) == 0
    for bad in (0, 9, 0x101, 0x10000 + 10 ** 6):
        err(indexed(L, [1], [0], bad), MPJX_ERR_ARG, b"unknown or freed datatype code %d" % bad)
        err(hvector(L, 2, 1, 2, bad), MPJX_ERR_ARG, b"%d" % bad)
    err(indexed(L, [1 << 61], [0], DOUBLE), MPJX_ERR_ARG, b"2^62")
    err(hindexed(L, [1], [1 << 61], DOUBLE), MPJX_ERR_ARG, b"2^62")
    err(hvector(L, 1 << 40, 1, 1 << 40, DOUBLE), MPJX_ERR_ARG, b"2^62")
    err(indexed(L, [1, 1], [3, -2], INT), MPJX_ERR_UNSUPPORTED, b"negative displacement", b"-2", b"index 1")
    err(indexed(L, [1], [-1], DOUBLE2), MPJX_ERR_UNSUPPORTED, b"-2 base elements")  # in units of the pair
    err(hvector(L, 2, 1, 0, INT), MPJX_ERR_UNSUPPORTED, b"stride 0", b"count 2")
    err(hvector(L, 3, 1, -4, INT), MPJX_ERR_UNSUPPORTED, b"stride -4")
    assert made(hvector(L, 1, 2, -4, INT)) >= 0x10000  # one block: the stride does not matter


def test_one_block_too_many(L):
    n = (1 << 20) + 1
    bl, disp = [1] * n, list(range(0, 2 * n, 2))
    r = indexed(L, bl, disp, BYTE)
    assert r == (MPJX_ERR_UNSUPPORTED, -1)
    assert b"1048576 blocks" in L.mpjx_last_error()
    code = made(indexed(L, bl[:-1], [d + 1 for d in disp[:-1]], BYTE))  # 2^20 unit blocks are a type
    assert layout(L, code) == (BYTE, n - 1, 2 * (n - 1) - 1, 1, 2 * (n - 1), n - 1, 0)
    assert L.mpjx_type_free(code) == 0


def test_use_after_free_and_codes_are_not_reissued(L):
    t = made(indexed(L, [2, 1], [9, 4], INT))
    assert L.mpjx_type_free(t) == 0 and L.mpjx_type_free(t) == MPJX_ERR_ARG
    code = ctypes.c_int(-1)
    base = ctypes.c_int()
    assert L.mpjx_type_info(t, ctypes.byref(base), None, None) == MPJX_ERR_ARG
    assert L.mpjx_type_layout(t, None, None, None, None) == MPJX_ERR_ARG
    assert indexed(L, [1], [0], t)[0] == MPJX_ERR_ARG and hvector(L, 2, 1, 9, t)[0] == MPJX_ERR_ARG
    assert L.mpjx_type_vector(2, 1, 2, t, ctypes.byref(code)) == MPJX_ERR_ARG
    later = [made(hindexed(L, [2, 1], [9, 4], INT)) for _ in range(8)]
    assert t not in later and len(set(later)) == 8 and min(later) > t
    for x in later:
        assert L.mpjx_type_free(x) == 0


def test_older_entry_points_still_reject_the_new_codes(L):
    t = made(indexed(L, [2, 1], [9, 4], INT))
    assert L.mpjx_type_size(t) == 0
    assert L.mpjx_op_check(3, t) == MPJX_ERR_ARG
    tab = (ctypes.c_int64 * 1)(0)
    assert L.mpjx_alltoallv(None, None, tab, tab, None, tab, tab, t, None) == MPJX_ERR_ARG
    assert L.mpjx_alltoallv_dt(None, None, tab, tab, t, None, tab, tab, t, None) == MPJX_ERR_ARG
    assert L.mpjx_type_free(t) == 0


def test_python_mirror_types():
    from mpjexpress_amd.mpi import MPI, Datatype, MPIException

    a = Datatype.Indexed([2, 1], [9, 4], MPI.INT)
    assert (a.Size(), a.Extent(), a.Lb(), a.Ub(), a.baseType, a.derived) == (3, 7, 4, 11, 5, True)
    a.Commit()
    h = Datatype.Hindexed([2, 1], [18, 8], MPI.DOUBLE2)
    assert (h.Size(), h.Extent(), h.Lb(), h.Ub(), h.baseType, h.byteSize) == (6, 14, 8, 22, 8, 48)
    v = Datatype.Vector(2, 3, 4, MPI.INT)
    hv = Datatype.Hvector(3, 1, 9, v)
    assert (hv.Size(), hv.Extent(), hv.Lb(), hv.Ub()) == (18, 25, 0, 25)
    assert (v.Lb(), v.Ub(), MPI.DOUBLE2.Lb(), MPI.DOUBLE2.Ub(), MPI.INT.Ub()) == (0, 7, 0, 2, 1)
    with pytest.raises(MPIException, match=r"\(-6\).*negative displacement"):
        Datatype.Indexed([1], [-1], MPI.INT)
    with pytest.raises(MPIException, match=r"\(-1\)"):
        Datatype.Hindexed([-1], [0], MPI.INT)
    with pytest.raises(MPIException, match=r"\(-6\).*stride 0"):
        Datatype.Hvector(2, 1, 0, MPI.INT)
    with pytest.raises(MPIException, match="2 block lengths but 1 displacements"):
        Datatype.Indexed([1, 1], [0], MPI.INT)
    for t in (a, h, hv, v):
        t.Free()
    with pytest.raises(MPIException, match=r"\(-1\)"):
        Datatype.Hvector(2, 1, 9, a)


def test_planner_under_sanitizers(tmp_path):
    build_and_run(tmp_path, "indexed_plan_test", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_registry_under_concurrent_create_and_free(tmp_path):
    build_and_run(tmp_path, "indexed_registry_test", ["-fsanitize=thread"], extra=("-pthread",))
