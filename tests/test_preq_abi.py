"""CPU: the persistent requests' ABI surface, their host side and k_msgs_pool's launch index (no GPU).

  - include/mpjx.h declares the six prototypes verbatim, libmpjx exports them and the ctypes table binds them.
  - Argument errors, none of which needs a device: a NULL request, a negative count and a negative tag (checked
    before the communicator is looked at), a NULL communicator, mpjx_start on a NULL handle, mpjx_startall with
    n < 0 or a NULL list. A bad rank and mpjx_start on a handle of mpjx_irecv need a world and are in
    tests/test_gpu_preq.py.
  - tests/cpp/preq_plan_test.cpp (Persist's lifecycle over 1,000 rounds from 8 threads, array-order posting,
    free while active, the pool map) is compiled with plain g++ and run as a stand-alone program under
    AddressSanitizer + UBSan and under ThreadSanitizer; tests/cpp/msgs_pool_plan_test.cpp (the launch index for
    both tile sizes and the shared per-lane mapping, every packed byte) under AddressSanitizer + UBSan.
"""
import ctypes
import os
import re
import subprocess

import pytest

from test_p2p_abi import ASAN, build_and_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "mpjx.h")
MPJX_ERR_ARG = -1
INT = 5

PROTOTYPES = """
int mpjx_send_init(mpjx_comm_t comm, const void *buf, int64_t count, int type, int dest, int tag,
                   mpjx_request_t *request);
int mpjx_recv_init(mpjx_comm_t comm, void *buf, int64_t count, int type, int source, int tag,
                   mpjx_request_t *request);
int mpjx_start(mpjx_request_t *request);
int mpjx_startall(int n, mpjx_request_t *requests);
int mpjx_request_is_persistent(mpjx_request_t request, int *persistent, int *active);
int mpjx_comm_p2p_pool_stats(mpjx_comm_t comm, int64_t *pool_launches, int64_t *puts, int64_t *hits,
                             int64_t *slots_in_use, int *batch_max);
"""
NEW = re.findall(r"^int (mpjx_[a-z0-9_]+)\(", PROTOTYPES, re.M)


@pytest.fixture(scope="module")
def L():
    from mpjexpress_amd import _lib

    return _lib.lib()


def test_header_declares_every_prototype_verbatim():
    assert len(NEW) == 6
    txt = open(HDR).read()
    assert PROTOTYPES.strip() in txt
    assert "persistent requests, Waitany" not in txt  # no longer listed as missing


def test_library_exports_and_binds_them(L):
    from mpjexpress_amd import _lib

    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for f in NEW:
        assert f in exported, f
        assert f in _lib.BOUND, f
        assert getattr(L, f).restype is ctypes.c_int and getattr(L, f).argtypes is not None, f


def test_err_arg_cases_need_no_device(L):
    """What mpjx_send_init / mpjx_recv_init can judge from the arguments alone they judge before they look at the
    communicator: a NULL request, a negative count, a negative tag. A bad rank needs the communicator's size and
    mpjx_start on a handle of mpjx_irecv needs a world: tests/test_gpu_preq.py::test_init_and_start_argument_errors."""
    h = ctypes.c_void_p(0xdead)
    for init in (L.mpjx_send_init, L.mpjx_recv_init):
        assert init(None, None, 0, INT, 0, 0, None) == MPJX_ERR_ARG and b"request is NULL" in L.mpjx_last_error()
        for call, msg in ((lambda: init(None, None, -1, INT, 0, 0, ctypes.byref(h)), b"negative count -1"),
                          (lambda: init(None, None, 0, INT, 0, -1, ctypes.byref(h)), b"tag -1 is negative"),
                          (lambda: init(None, None, 0, INT, 0, -7, ctypes.byref(h)), b"tag -7 is negative"),
                          (lambda: init(None, None, 0, INT, 0, 0, ctypes.byref(h)), b"comm is NULL")):
            h.value = 0xdead
            assert call() == MPJX_ERR_ARG and msg in L.mpjx_last_error(), (msg, L.mpjx_last_error())
            assert not h.value  # the handle is NULL after any failure
    # ANY_TAG is a send's error and a receive's right: the receive gets as far as the communicator
    assert L.mpjx_send_init(None, None, 0, INT, 0, -2, ctypes.byref(h)) == MPJX_ERR_ARG and b"negative" in L.mpjx_last_error()
    assert L.mpjx_recv_init(None, None, 0, INT, 0, -2, ctypes.byref(h)) == MPJX_ERR_ARG and b"comm is NULL" in L.mpjx_last_error()
    assert L.mpjx_comm_p2p_pool_stats(None, None, None, None, None, None) == MPJX_ERR_ARG
    assert b"comm is NULL" in L.mpjx_last_error()
    # Start: a NULL pointer, a NULL handle
    h = ctypes.c_void_p()
    assert L.mpjx_start(None) == MPJX_ERR_ARG
    assert L.mpjx_start(ctypes.byref(h)) == MPJX_ERR_ARG and b"NULL" in L.mpjx_last_error()
    assert not h.value
    # Startall: n < 0, a NULL list with n > 0; an empty list and a list of NULL handles post nothing
    hs = (ctypes.c_void_p * 3)()
    assert L.mpjx_startall(-1, hs) == MPJX_ERR_ARG
    assert L.mpjx_startall(2, None) == MPJX_ERR_ARG
    assert L.mpjx_startall(0, None) == 0 and L.mpjx_startall(3, hs) == 0
    # a NULL handle is neither persistent nor active; the out pointers are optional
    p, a = ctypes.c_int(7), ctypes.c_int(7)
    assert L.mpjx_request_is_persistent(None, ctypes.byref(p), ctypes.byref(a)) == 0 and (p.value, a.value) == (0, 0)
    assert L.mpjx_request_is_persistent(None, None, None) == 0


def test_python_mirror_surface():
    from mpjexpress_amd.mpi import Intracomm, Prequest, Request

    assert issubclass(Prequest, Request)
    for m in ("Send_init", "Recv_init", "p2p_pool_stats"):
        assert callable(getattr(Intracomm, m)), m
    for m in ("Start", "Startall", "Wait", "Test", "Free", "Is_null", "Waitall"):
        assert callable(getattr(Prequest, m)), m
    assert Prequest(None, None, None).Is_null()
    Prequest.Startall([])


def test_cpp_mirror_has_prequest(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "mpjx.hpp"\n'
                   'int main(){ std::vector<mpi::Prequest> v; mpi::Prequest::Startall(v);\n'
                   '  auto st = mpi::Request::Waitall(v); mpi::Prequest p; return (p.Is_null() && st.empty()) ? 0 : 1; }\n')
    lib = os.path.join(ROOT, "mpjexpress_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "t"), f"-L{lib}", "-lmpjx", f"-Wl,-rpath,{lib}"])
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def test_persistent_host_side_under_asan_and_ubsan(tmp_path):
    build_and_run(tmp_path, "preq_plan_test", ASAN, extra=("-pthread",))


def test_persistent_host_side_under_tsan(tmp_path):
    build_and_run(tmp_path, "preq_plan_test", ["-fsanitize=thread"], extra=("-pthread",))


def test_pool_index_planner_under_asan_and_ubsan(tmp_path):
    build_and_run(tmp_path, "msgs_pool_plan_test", ASAN)
