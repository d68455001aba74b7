"""CPU: the derived datatypes' and the strided block move's ABI surface and host-side planner (no GPU).

  - include/mpjx.h declares mpjx_type_contiguous, mpjx_type_vector, mpjx_type_free, mpjx_type_info and
    mpjx_alltoallv_dt, libmpjx exports them, the ctypes table binds them, and mpjx_alltoallv_dt answers a NULL
    communicator with MPJX_ERR_ARG before touching anything.
  - mpjx_type_info on basic, pair and derived codes; normalisation; the MPJX_ERR_ARG and MPJX_ERR_UNSUPPORTED
    cases; use after free; the existing entry points keep rejecting derived codes.
  - tests/cpp/strided_plan_test.cpp, a stand-alone program over mpjexpress_amd/csrc/mpjx_strided_plan.hpp, is
    compiled with plain g++ under AddressSanitizer and UBSan and run; tests/cpp/type_registry_test.cpp, the
    registry under concurrent create / free from 8 threads, under ThreadSanitizer where that links and starts.
"""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "mpjx.h")
NEW = ("mpjx_type_contiguous", "mpjx_type_vector", "mpjx_type_free", "mpjx_type_info", "mpjx_alltoallv_dt")
MPJX_ERR_ARG, MPJX_ERR_UNSUPPORTED = -1, -6
BYTE, INT, DOUBLE, DOUBLE2 = 1, 5, 8, 0x108


@pytest.fixture(scope="module")
def L():
    from mpjexpress_amd import _lib

    return _lib.lib()


def info(L, code):
    base, size, extent = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()
    rc = L.mpjx_type_info(code, ctypes.byref(base), ctypes.byref(size), ctypes.byref(extent))
    return rc, base.value, size.value, extent.value


def vector(L, count, blocklength, stride, old):
    code = ctypes.c_int(-1)
    return L.mpjx_type_vector(count, blocklength, stride, old, ctypes.byref(code)), code.value


def contiguous(L, count, old):
    code = ctypes.c_int(-1)
    return L.mpjx_type_contiguous(count, old, ctypes.byref(code)), code.value


def test_header_declares_the_five_functions():
    txt = open(HDR).read()
    fns = set(re.findall(r"^int\s+(mpjx_[a-z_]+)\(", txt, re.M))
    for f in NEW:
        assert f in fns, f
    m = re.search(r"int mpjx_alltoallv_dt\(([^;]*)\);", txt)
    args = " ".join(m.group(1).split())
    assert args == ("mpjx_comm_t comm, const void *sendbuf, const int64_t *sendcounts, const int64_t *sdispls, "
                    "int sendtype, void *recvbuf, const int64_t *recvcounts, const int64_t *rdispls, int recvtype, "
                    "void *stream")
    assert re.search(r"int mpjx_type_vector\(int64_t count, int64_t blocklength, int64_t stride, int oldtype, "
                     r"int \*newtype\);", txt)
    assert "65,536 blocks" in txt  # where the exact overlap check stops is part of the contract


def test_library_exports_and_binds_them(L):
    from mpjexpress_amd import _lib

    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for f in NEW:
        assert f in exported, f
        assert f in _lib.EXPORTS, f
        assert getattr(L, f).restype is ctypes.c_int


def test_null_communicator_is_err_arg(L):
    tab = (ctypes.c_int64 * 1)(0)
    assert L.mpjx_alltoallv_dt(None, None, tab, tab, INT, None, tab, tab, INT, None) == MPJX_ERR_ARG
    assert b"comm is NULL" in L.mpjx_last_error()


def test_type_info_on_basic_and_pair_codes(L):
    assert info(L, BYTE) == (0, BYTE, 1, 1)
    assert info(L, DOUBLE) == (0, DOUBLE, 1, 1)
    assert info(L, DOUBLE2) == (0, DOUBLE, 2, 2)
    assert info(L, 0x103) == (0, 3, 2, 2)
    for bad in (0, 9, 0x101, 0x104, 0x10000 + 10 ** 6, -1):
        assert info(L, bad)[0] == MPJX_ERR_ARG, bad
    assert L.mpjx_type_info(INT, None, None, None) == 0  # every out pointer is optional


def test_vector_and_its_normal_form(L):
    rc, v = vector(L, 6, 2, 5, INT)
    assert rc == 0 and v >= 0x10000
    assert info(L, v) == (0, INT, 12, 27)  # (6 - 1) * 5 + 2
    rc, w = vector(L, 4, 3, 3, INT)  # stride == blocklength: contiguous
    assert rc == 0 and w != v and info(L, w) == (0, INT, 12, 12)
    rc, one = vector(L, 1, 3, -7, INT)  # one block: the stride does not matter
    assert rc == 0 and info(L, one) == (0, INT, 3, 3)
    rc, none = vector(L, 0, 3, 7, INT)
    assert rc == 0 and info(L, none) == (0, INT, 0, 0)
    rc, hollow = vector(L, 5, 0, 7, INT)
    assert rc == 0 and info(L, hollow) == (0, INT, 0, 0)
    rc, pairs = vector(L, 3, 2, 4, DOUBLE2)  # blocklength and stride in pairs
    assert rc == 0 and info(L, pairs) == (0, DOUBLE, 12, 20)
    rc, c4 = contiguous(L, 4, INT)
    assert rc == 0 and info(L, c4) == (0, INT, 4, 4)
    rc, over = vector(L, 3, 2, 5, c4)  # a contiguous derived oldtype: units of 4 ints
    assert rc == 0 and info(L, over) == (0, INT, 24, 48)
    rc, over2 = vector(L, 2, 1, 2, w)  # ... and a Vector that normalised to contiguous
    assert rc == 0 and info(L, over2) == (0, INT, 24, 36)
    rc, cc = contiguous(L, 2, DOUBLE2)
    assert rc == 0 and info(L, cc) == (0, DOUBLE, 4, 4)
    for t in (v, w, one, none, hollow, pairs, c4, over, over2, cc):
        assert L.mpjx_type_free(t) == 0


def test_err_arg_and_err_unsupported(L):
    assert vector(L, -1, 2, 5, INT)[0] == MPJX_ERR_ARG
    assert vector(L, 2, -1, 5, INT)[0] == MPJX_ERR_ARG
    assert contiguous(L, -1, INT)[0] == MPJX_ERR_ARG
    assert vector(L, 2, 1, 2, 0)[0] == MPJX_ERR_ARG and contiguous(L, 2, 77)[0] == MPJX_ERR_ARG
    assert L.mpjx_type_vector(2, 1, 2, INT, None) == MPJX_ERR_ARG
    assert vector(L, 2, 1 << 61, 1 << 62, DOUBLE)[0] == MPJX_ERR_ARG
    for stride, word in ((2, b"stride 2"), (0, b"stride 0"), (-4, b"stride -4")):  # overlapping, zero, negative
        assert vector(L, 2, 3, stride, INT)[0] == MPJX_ERR_UNSUPPORTED
        msg = L.mpjx_last_error()
        assert word in msg and b"blocklength 3" in msg, msg
    rc, v = vector(L, 6, 2, 5, INT)
    assert rc == 0
    assert vector(L, 2, 1, 2, v)[0] == MPJX_ERR_UNSUPPORTED  # Vector of Vector
    assert b"6 blocks of 2 at stride 5" in L.mpjx_last_error()
    assert contiguous(L, 2, v)[0] == MPJX_ERR_UNSUPPORTED  # Contiguous of Vector
    assert L.mpjx_type_free(v) == 0


def test_use_after_free_and_codes_are_not_reissued(L):
    rc, v = vector(L, 6, 2, 5, INT)
    assert rc == 0 and L.mpjx_type_free(v) == 0
    assert L.mpjx_type_free(v) == MPJX_ERR_ARG
    assert info(L, v)[0] == MPJX_ERR_ARG
    assert vector(L, 2, 1, 1, v)[0] == MPJX_ERR_ARG and contiguous(L, 2, v)[0] == MPJX_ERR_ARG
    later = [vector(L, 6, 2, 5, INT)[1] for _ in range(8)]
    assert v not in later and len(set(later)) == 8 and min(later) > v
    for t in later:
        assert L.mpjx_type_free(t) == 0
    assert L.mpjx_type_free(INT) == MPJX_ERR_ARG and L.mpjx_type_free(DOUBLE2) == MPJX_ERR_ARG


def test_existing_entry_points_still_reject_derived_codes(L):
    rc, v = vector(L, 6, 2, 5, INT)
    assert rc == 0
    assert L.mpjx_type_size(v) == 0
    assert L.mpjx_op_check(3, v) == MPJX_ERR_ARG
    # with a communicator, mpjx_alltoallv(..., type = derived) is MPJX_ERR_ARG through that same test:
    # tests/test_gpu_strided.py::test_existing_alltoallv_still_rejects_a_derived_code
    tab = (ctypes.c_int64 * 1)(0)
    assert L.mpjx_alltoallv(None, None, tab, tab, None, tab, tab, v, None) == MPJX_ERR_ARG
    assert L.mpjx_type_free(v) == 0


def test_python_mirror_types():
    from mpjexpress_amd.mpi import MPI, Datatype, MPIException

    v = Datatype.Vector(3, 2, 4, MPI.DOUBLE2)
    assert (v.Size(), v.Extent(), v.Lb(), v.Ub(), v.baseType, v.derived) == (12, 20, 0, 20, 8, True)
    assert v.code >= 0x10000 and v.byteSize == 96
    v.Commit()
    c = Datatype.Contiguous(4, MPI.INT)
    assert (c.Size(), c.Extent()) == (4, 4)
    assert (MPI.INT.Size(), MPI.INT.Extent(), MPI.DOUBLE2.Extent(), MPI.INT.derived) == (1, 1, 2, False)
    with pytest.raises(MPIException, match=r"\(-6\)"):
        Datatype.Vector(2, 3, 2, MPI.INT)
    with pytest.raises(MPIException, match=r"\(-1\)"):
        Datatype.Vector(-2, 3, 4, MPI.INT)
    v.Free()
    c.Free()
    with pytest.raises(MPIException, match=r"\(-1\)"):
        Datatype.Contiguous(2, c)
    MPI.INT.Free()  # a basic type has nothing to release


def build_and_run(tmp_path, name, sanitize, extra=()):
    gxx = shutil.which("g++")
    assert gxx, f"g++ is needed to build tests/cpp/{name}.cpp"
    src = os.path.join(ROOT, "tests", "cpp", f"{name}.cpp")
    exe = str(tmp_path / name)
    base = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", src, "-o", exe, *extra]
    r = subprocess.run(base + sanitize, capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find|libasan|libubsan|libtsan", r.stderr):
        print("sanitizer runtimes absent: built without them\n" + r.stderr[-500:])
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    if r.returncode != 0 and "Sanitizer: unexpected memory mapping" in r.stderr:
        # the sanitizer's runtime cannot lay out its shadow memory under this kernel's address-space
        # randomisation and exits before main(): the program itself never ran
        print("sanitizer runtime cannot start here: built without it\n" + r.stderr[-500:])
        assert subprocess.run(base, capture_output=True, text=True).returncode == 0
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and f"{name}: ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


def test_planner_under_sanitizers(tmp_path):
    build_and_run(tmp_path, "strided_plan_test", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_registry_under_concurrent_create_and_free(tmp_path):
    build_and_run(tmp_path, "type_registry_test", ["-fsanitize=thread"], extra=("-pthread",))
