"""CPU: the point-to-point calls' ABI surface, the matching engine and k_msgs' planner (no GPU).

  - include/mpjx.h declares the thirteen prototypes verbatim, libmpjx exports them, the ctypes table binds them,
    and each answers a NULL communicator (or a NULL request) with MPJX_ERR_ARG before touching anything.
  - mpjx_get_count on hand-made statuses: Comm.java:1517-1531.
  - tests/cpp/p2p_match_test.cpp (the mailbox, the eager slab, 8 threads x 10,000 envelopes) and
    tests/cpp/msgs_plan_test.cpp (the launch table and both kinds' address mapping, every packed byte) are
    compiled with plain g++ under AddressSanitizer and UBSan and run; the first also under ThreadSanitizer where
    that links and starts.
"""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "mpjx.h")
MPJX_ERR_ARG, MPJX_UNDEFINED = -1, -1
INT, INT2, LB = 5, 0x105, 10

PROTOTYPES = """
typedef struct mpjx_request *mpjx_request_t;
typedef struct { int source, tag, error; int64_t elements, bytes; } mpjx_status;

int mpjx_isend(mpjx_comm_t comm, const void *buf, int64_t count, int type, int dest, int tag,
               mpjx_request_t *request);
int mpjx_irecv(mpjx_comm_t comm, void *buf, int64_t count, int type, int source, int tag,
               mpjx_request_t *request);
int mpjx_send(mpjx_comm_t comm, const void *buf, int64_t count, int type, int dest, int tag);
int mpjx_recv(mpjx_comm_t comm, void *buf, int64_t count, int type, int source, int tag,
              mpjx_status *status);
int mpjx_sendrecv(mpjx_comm_t comm, const void *sendbuf, int64_t sendcount, int sendtype, int dest,
                  int sendtag, void *recvbuf, int64_t recvcount, int recvtype, int source,
                  int recvtag, mpjx_status *status);
int mpjx_sendrecv_replace(mpjx_comm_t comm, void *buf, int64_t count, int type, int dest,
                          int sendtag, int source, int recvtag, mpjx_status *status);
int mpjx_wait(mpjx_request_t *request, mpjx_status *status);
int mpjx_test(mpjx_request_t *request, int *flag, mpjx_status *status);
int mpjx_waitall(int n, mpjx_request_t *requests, mpjx_status *statuses);
int mpjx_request_free(mpjx_request_t *request);
int mpjx_get_count(const mpjx_status *status, int type, int64_t *count, int64_t *elements);
int mpjx_comm_set_p2p_timeout(mpjx_comm_t comm, double seconds);
int mpjx_comm_p2p_stats(mpjx_comm_t comm, int64_t *launches, int64_t *moved, int64_t *eager,
                        int *table_max);
"""
NEW = re.findall(r"^int (mpjx_[a-z0-9_]+)\(", PROTOTYPES, re.M)


@pytest.fixture(scope="module")
def L():
    from mpjexpress_amd import _lib

    return _lib.lib()


def test_header_declares_every_prototype_verbatim():
    assert len(NEW) == 13
    txt = open(HDR).read()
    assert PROTOTYPES.strip() in txt
    for name, val in (("MPJX_ANY_SOURCE", -2), ("MPJX_ANY_TAG", -2), ("MPJX_PROC_NULL", -3), ("MPJX_UNDEFINED", -1)):
        assert re.search(rf"\b{name} = {val}\b", txt), name


def test_library_exports_and_binds_them(L):
    from mpjexpress_amd import _lib

    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for f in NEW:
        assert f in exported, f
        assert f in _lib.BOUND, f
        assert getattr(L, f).restype is ctypes.c_int and getattr(L, f).argtypes is not None, f
    assert ctypes.sizeof(_lib.Status) == 32  # three ints, padding, two int64


def test_null_communicator_is_err_arg(L):
    from mpjexpress_amd import _lib

    h, st = ctypes.c_void_p(), _lib.Status()
    calls = [
        lambda: L.mpjx_isend(None, None, 0, INT, 0, 0, ctypes.byref(h)),
        lambda: L.mpjx_irecv(None, None, 0, INT, 0, 0, ctypes.byref(h)),
        lambda: L.mpjx_send(None, None, 0, INT, 0, 0),
        lambda: L.mpjx_recv(None, None, 0, INT, 0, 0, ctypes.byref(st)),
        lambda: L.mpjx_sendrecv(None, None, 0, INT, 0, 0, None, 0, INT, 0, 0, ctypes.byref(st)),
        lambda: L.mpjx_sendrecv_replace(None, None, 0, INT, 0, 0, 0, 0, ctypes.byref(st)),
        lambda: L.mpjx_comm_set_p2p_timeout(None, 1.0),
        lambda: L.mpjx_comm_p2p_stats(None, None, None, None, None),
    ]
    for i, f in enumerate(calls):
        assert f() == MPJX_ERR_ARG, i
        assert b"comm is NULL" in L.mpjx_last_error(), i
    assert L.mpjx_wait(None, None) == MPJX_ERR_ARG and L.mpjx_request_free(None) == MPJX_ERR_ARG
    assert L.mpjx_test(None, None, None) == MPJX_ERR_ARG and L.mpjx_waitall(2, None, None) == MPJX_ERR_ARG
    # a NULL request is complete: an empty status
    flag = ctypes.c_int(0)
    assert L.mpjx_wait(ctypes.byref(h), ctypes.byref(st)) == 0 and (st.source, st.tag, st.elements) == (-3, -2, 0)
    assert L.mpjx_test(ctypes.byref(h), ctypes.byref(flag), None) == 0 and flag.value == 1
    assert L.mpjx_waitall(0, None, None) == 0 and L.mpjx_request_free(ctypes.byref(h)) == 0


def get_count(L, elements, code):
    from mpjexpress_amd import _lib

    st = _lib.Status(1, 7, 0, elements, 0)
    c, e = ctypes.c_int64(-99), ctypes.c_int64(-99)
    rc = L.mpjx_get_count(ctypes.byref(st), code, ctypes.byref(c), ctypes.byref(e))
    return rc, c.value, e.value


def test_get_count(L):
    assert get_count(L, 50, INT) == (0, 50, 50)
    assert get_count(L, 5, INT2) == (0, MPJX_UNDEFINED, 5)  # 5 elements are not a whole number of pairs
    assert get_count(L, 6, INT2) == (0, 3, 6)
    # a type of size 0: count is what the status carries (the receive count), elements MPJX_UNDEFINED
    bl, ds, ts = (ctypes.c_int64 * 1)(1), (ctypes.c_int64 * 1)(0), (ctypes.c_int * 1)(LB)
    empty = ctypes.c_int(-1)
    assert L.mpjx_type_struct(1, bl, ds, ts, ctypes.byref(empty)) == 0
    assert get_count(L, 4, empty.value) == (0, 4, MPJX_UNDEFINED)
    assert L.mpjx_type_free(empty.value) == 0
    assert get_count(L, 4, empty.value)[0] == MPJX_ERR_ARG  # freed
    assert L.mpjx_get_count(None, INT, None, None) == MPJX_ERR_ARG
    from mpjexpress_amd import _lib
    assert L.mpjx_get_count(ctypes.byref(_lib.Status()), INT, None, None) == 0  # the out pointers are optional


def test_python_mirror_surface():
    from mpjexpress_amd import _lib
    from mpjexpress_amd.mpi import MPI, Intracomm, Request, Status

    assert (MPI.ANY_SOURCE, MPI.ANY_TAG, MPI.PROC_NULL, MPI.UNDEFINED) == (-2, -2, -3, -1)
    for m in ("Send", "Recv", "Isend", "Irecv", "Sendrecv", "Sendrecv_replace"):
        assert callable(getattr(Intracomm, m)), m
    for m in ("Wait", "Test", "Is_null", "Free", "Waitall"):
        assert callable(getattr(Request, m)), m
    st = Status(_lib.Status(2, 9, 0, 50, 200))
    assert (st.source, st.tag, st.Get_count(MPI.INT), st.Get_elements(MPI.INT)) == (2, 9, 50, 50)
    assert Status(_lib.Status(2, 9, 0, 5, 20)).Get_count(MPI.INT2) == MPI.UNDEFINED
    assert Request(None, None, None).Is_null() and Request.Waitall([]) == []


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


ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_matching_engine_under_asan_and_ubsan(tmp_path):
    build_and_run(tmp_path, "p2p_match_test", ASAN, extra=("-pthread",))


def test_matching_engine_under_tsan(tmp_path):
    build_and_run(tmp_path, "p2p_match_test", ["-fsanitize=thread"], extra=("-pthread",))


def test_msgs_planner_under_asan_and_ubsan(tmp_path):
    build_and_run(tmp_path, "msgs_plan_test", ASAN)
