"""ctypes binding of libmpjx.so (include/mpjx.h).

The library is built in-tree (mpjexpress_amd/lib/libmpjx.so, `make -C mpjexpress_amd`). There is no
CPU fallback: if the library is missing or cannot load, every entry point raises.
"""
import ctypes
import os

# torch (when present) must be loaded BEFORE libmpjx: both resolve libamdhip64.so.7 / librccl.so.1 by
# soname, and loading torch first makes libmpjx bind to the HIP runtime torch already mapped instead
# of mapping a second copy from /opt/rocm.
try:  # pragma: no cover - environment dependent
    import torch  # noqa: F401
except Exception:  # noqa: BLE001
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
# MPJX_LIB_PATH: another build of the same library (A/B timing of two builds in one GPU job)
LIB_PATH = os.environ.get("MPJX_LIB_PATH") or os.path.join(_HERE, "lib", "libmpjx.so")

_lib = None


class MPJXError(RuntimeError):
    """Raised for a non-zero libmpjx status (maps to mpi.MPIException on the Java side)."""

    def __init__(self, status, fn, detail):
        self.status = status
        super().__init__(f"{fn}: {strerror(status)} ({status}): {detail}")


class Status(ctypes.Structure):
    """mpjx_status (include/mpjx.h)."""
    _fields_ = [("source", ctypes.c_int), ("tag", ctypes.c_int), ("error", ctypes.c_int),
                ("elements", ctypes.c_int64), ("bytes", ctypes.c_int64)]


def _declare(L):
    c_int, c_i64, vp, c_uint = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_uint
    pi64 = ctypes.POINTER(ctypes.c_int64)
    sig = {
        "mpjx_version": ([], c_int),
        "mpjx_runtime_versions": ([ctypes.POINTER(c_int), ctypes.POINTER(c_int)], c_int),
        "mpjx_strerror": ([c_int], ctypes.c_char_p),
        "mpjx_last_error": ([], ctypes.c_char_p),
        "mpjx_type_size": ([c_int], c_int),
        "mpjx_op_check": ([c_int, c_int], c_int),
        "mpjx_device_count": ([ctypes.POINTER(c_int)], c_int),
        "mpjx_combine": ([c_int, c_int, vp, vp, c_i64, vp], c_int),
        "mpjx_combine_multi": ([c_int, c_int, c_int, c_int, ctypes.POINTER(vp), ctypes.POINTER(vp), c_i64,
                                c_int, c_uint, vp], c_int),
        "mpjx_mpjbuf_section": ([vp, c_i64, c_i64, ctypes.POINTER(c_int), pi64, pi64], c_int),
        "mpjx_mpjbuf_combine": ([c_int, c_int, vp, vp, c_i64, c_i64, vp, c_uint, vp], c_int),
        "mpjx_get_unique_id": ([ctypes.c_char_p], c_int),
        "mpjx_comm_init_rank": ([ctypes.POINTER(vp), c_int, ctypes.c_char_p, c_int, c_int], c_int),
        "mpjx_comm_init_smp": ([ctypes.POINTER(vp), c_int, ctypes.POINTER(c_int)], c_int),
        "mpjx_comm_init_smp_rank": ([ctypes.POINTER(vp), c_int, ctypes.c_char_p, c_int, ctypes.POINTER(c_int)],
                                    c_int),
        "mpjx_comm_init_ipc": ([ctypes.POINTER(vp), c_int, ctypes.c_char_p, c_int, c_int], c_int),
        "mpjx_comm_destroy": ([vp], c_int),
        "mpjx_comm_rank": ([vp, ctypes.POINTER(c_int)], c_int),
        "mpjx_comm_size": ([vp, ctypes.POINTER(c_int)], c_int),
        "mpjx_comm_device": ([vp, ctypes.POINTER(c_int)], c_int),
        "mpjx_comm_stream": ([vp, ctypes.POINTER(vp)], c_int),
        "mpjx_comm_synchronize": ([vp], c_int),
        "mpjx_barrier": ([vp], c_int),
        "mpjx_comm_phase_timing": ([vp, c_int], c_int),
        "mpjx_comm_last_phases": ([vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(c_int)], c_int),
        "mpjx_comm_pipeline_trace": ([vp, ctypes.POINTER(ctypes.c_float), c_int, ctypes.POINTER(c_int)], c_int),
        "mpjx_reduce": ([vp, vp, vp, c_i64, c_int, c_int, c_int, c_uint, vp], c_int),
        "mpjx_allreduce": ([vp, vp, vp, c_i64, c_int, c_int, c_uint, vp], c_int),
        "mpjx_reduce_scatter": ([vp, vp, vp, pi64, c_int, c_int, c_uint, vp], c_int),
        "mpjx_scan": ([vp, vp, vp, c_i64, c_int, c_int, c_uint, vp], c_int),
        "mpjx_bcast": ([vp, vp, c_i64, c_int, c_int, vp], c_int),
        "mpjx_gather": ([vp, vp, vp, c_i64, c_int, c_int, vp], c_int),
        "mpjx_scatter": ([vp, vp, vp, c_i64, c_int, c_int, vp], c_int),
        "mpjx_allgather": ([vp, vp, vp, c_i64, c_int, vp], c_int),
        "mpjx_allgatherv": ([vp, vp, c_i64, vp, pi64, pi64, c_int, vp], c_int),
        "mpjx_gatherv": ([vp, vp, c_i64, vp, pi64, pi64, c_int, c_int, vp], c_int),
        "mpjx_scatterv": ([vp, vp, pi64, pi64, vp, c_i64, c_int, c_int, vp], c_int),
        "mpjx_alltoall": ([vp, vp, vp, c_i64, c_int, vp], c_int),
        "mpjx_alltoallv": ([vp, vp, pi64, pi64, vp, pi64, pi64, c_int, vp], c_int),
        "mpjx_type_contiguous": ([c_i64, c_int, ctypes.POINTER(c_int)], c_int),
        "mpjx_type_vector": ([c_i64, c_i64, c_i64, c_int, ctypes.POINTER(c_int)], c_int),
        "mpjx_type_hvector": ([c_i64, c_i64, c_i64, c_int, ctypes.POINTER(c_int)], c_int),
        "mpjx_type_indexed": ([c_int, pi64, pi64, c_int, ctypes.POINTER(c_int)], c_int),
        "mpjx_type_hindexed": ([c_int, pi64, pi64, c_int, ctypes.POINTER(c_int)], c_int),
        "mpjx_type_layout": ([c_int, pi64, pi64, pi64, ctypes.POINTER(c_int)], c_int),
        "mpjx_type_struct": ([c_int, pi64, pi64, ctypes.POINTER(c_int), ctypes.POINTER(c_int)], c_int),
        "mpjx_type_true_bounds": ([c_int, pi64, pi64], c_int),
        "mpjx_comm_last_move_kernels": ([vp, ctypes.POINTER(c_uint)], c_int),
        "mpjx_type_free": ([c_int], c_int),
        "mpjx_type_info": ([c_int, ctypes.POINTER(c_int), pi64, pi64], c_int),
        "mpjx_alltoallv_dt": ([vp, vp, pi64, pi64, c_int, vp, pi64, pi64, c_int, vp], c_int),
        "mpjx_reduce_dt": ([vp, vp, vp, c_i64, c_int, c_int, c_int, c_uint, vp], c_int),
        "mpjx_allreduce_dt": ([vp, vp, vp, c_i64, c_int, c_int, c_uint, vp], c_int),
        "mpjx_reduce_scatter_dt": ([vp, vp, vp, pi64, c_int, c_int, c_uint, vp], c_int),
        "mpjx_scan_dt": ([vp, vp, vp, c_i64, c_int, c_int, c_uint, vp], c_int),
        "mpjx_comm_last_dt_form": ([vp, ctypes.POINTER(c_int)], c_int),
        "mpjx_pack_size": ([c_i64, c_int, pi64], c_int),
        "mpjx_pack": ([vp, vp, c_i64, c_int, vp, c_i64, pi64, vp], c_int),
        "mpjx_unpack": ([vp, vp, c_i64, pi64, vp, c_i64, c_int, vp, vp], c_int),
        "mpjx_reduce_host": ([vp, vp, vp, c_i64, c_int, c_int, c_int, c_uint], c_int),
        "mpjx_allreduce_host": ([vp, vp, vp, c_i64, c_int, c_int, c_uint], c_int),
        "mpjx_reduce_scatter_host": ([vp, vp, vp, pi64, c_int, c_int, c_uint], c_int),
        "mpjx_scan_host": ([vp, vp, vp, c_i64, c_int, c_int, c_uint], c_int),
        "mpjx_host_alloc": ([ctypes.POINTER(vp), c_i64], c_int),
        "mpjx_host_free": ([vp], c_int),
        "mpjx_comm_last_host_form": ([vp, ctypes.POINTER(c_int)], c_int),
        "mpjx_isend": ([vp, vp, c_i64, c_int, c_int, c_int, ctypes.POINTER(vp)], c_int),
        "mpjx_irecv": ([vp, vp, c_i64, c_int, c_int, c_int, ctypes.POINTER(vp)], c_int),
        "mpjx_send": ([vp, vp, c_i64, c_int, c_int, c_int], c_int),
        "mpjx_recv": ([vp, vp, c_i64, c_int, c_int, c_int, ctypes.POINTER(Status)], c_int),
        "mpjx_sendrecv": ([vp, vp, c_i64, c_int, c_int, c_int, vp, c_i64, c_int, c_int, c_int,
                           ctypes.POINTER(Status)], c_int),
        "mpjx_sendrecv_replace": ([vp, vp, c_i64, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(Status)], c_int),
        "mpjx_wait": ([ctypes.POINTER(vp), ctypes.POINTER(Status)], c_int),
        "mpjx_test": ([ctypes.POINTER(vp), ctypes.POINTER(c_int), ctypes.POINTER(Status)], c_int),
        "mpjx_waitall": ([c_int, ctypes.POINTER(vp), ctypes.POINTER(Status)], c_int),
        "mpjx_request_free": ([ctypes.POINTER(vp)], c_int),
        "mpjx_get_count": ([ctypes.POINTER(Status), c_int, pi64, pi64], c_int),
        "mpjx_send_init": ([vp, vp, c_i64, c_int, c_int, c_int, ctypes.POINTER(vp)], c_int),
        "mpjx_recv_init": ([vp, vp, c_i64, c_int, c_int, c_int, ctypes.POINTER(vp)], c_int),
        "mpjx_start": ([ctypes.POINTER(vp)], c_int),
        "mpjx_startall": ([c_int, ctypes.POINTER(vp)], c_int),
        "mpjx_request_is_persistent": ([vp, ctypes.POINTER(c_int), ctypes.POINTER(c_int)], c_int),
        "mpjx_iprobe": ([vp, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(Status)], c_int),
        "mpjx_probe": ([vp, c_int, c_int, ctypes.POINTER(Status)], c_int),
        "mpjx_wire_bytes": ([ctypes.POINTER(Status), pi64], c_int),
    }
    # Bound like the rest but listed apart (BOUND, not EXPORTS): tests/test_abi.py compares EXPORTS with the names
    # its pattern finds in the header, and that pattern knows no digits
    more = {
        "mpjx_comm_set_p2p_timeout": ([vp, ctypes.c_double], c_int),
        "mpjx_comm_p2p_stats": ([vp, pi64, pi64, pi64, ctypes.POINTER(c_int)], c_int),
        "mpjx_comm_p2p_pool_stats": ([vp, pi64, pi64, pi64, pi64, ctypes.POINTER(c_int)], c_int),
        "mpjx_comm_p2p_wire_stats": ([vp, pi64, pi64, pi64, ctypes.POINTER(c_int)], c_int),
    }
    for name, (args, res) in list(sig.items()) + list(more.items()):
        f = getattr(L, name)
        f.argtypes = args
        f.restype = res
    return sig, more


EXPORTS = None
BOUND = None  # every function the table binds: EXPORTS and those whose names carry a digit


def lib():
    """Load libmpjx.so (once). Raises if it is not built — there is no fallback path."""
    global _lib, EXPORTS, BOUND
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"libmpjx.so not found at {LIB_PATH}: build it with `make -C mpjexpress_amd` "
                "(or __graft_entry__.build()); the HIP path has no CPU fallback")
        L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        sig, more = _declare(L)
        EXPORTS = sorted(sig)
        BOUND = sorted(list(sig) + list(more))
        _lib = L
    return _lib


def strerror(status):
    return lib().mpjx_strerror(status).decode()


def check(status, fn):
    if status != 0:
        detail = lib().mpjx_last_error().decode(errors="replace")
        raise MPJXError(status, fn, detail)
    return status


def call(name, *args):
    return check(getattr(lib(), name)(*args), name)
