"""Runs the block-move case matrix (tests/moves_cases.py) on rank threads in a fresh process.

    python tests/moves_driver.py smp|rccl P[,P...] TYPE[,TYPE...]

smp:  a multicore world on device 0 (the one-launch engine; MPJX_SMP_COPY=1 in the environment selects
      SmpTransport's exchanges).
rccl: P rank threads each form their rank of an "RCCL" world with mpjx_comm_init_rank. The caller points
      MPJX_LIB_PATH at tests/rccl/libmpjx_rccl_standin.so (tests/test_gpu_moves_standin.py does): the same
      libmpjx objects linked against the RCCL stand-in, so RcclTransport's allgather_equal, alltoallv and
      exchange carry the moves. The stand-in's log of the RCCL calls libmpjx made is reported.
Prints one JSON line: {"cases": n, "bad": [messages], "calls": {rccl call: count}}.
"""
import ctypes
import json
import os
import sys
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]

import torch  # noqa: E402

import moves_cases as MC  # noqa: E402
from mpjexpress_amd import _lib, mpi  # noqa: E402


def threads(P, body, limit=90):
    out, err = [None] * P, [None] * P

    def th(r):
        try:
            torch.cuda.set_device(0)
            out[r] = body(r)
        except BaseException as e:  # noqa: BLE001
            err[r] = f"{type(e).__name__}: {e}"
    ts = [threading.Thread(target=th, args=(r,), daemon=True) for r in range(P)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=limit)
    if any(t.is_alive() for t in ts):
        raise AssertionError("a rank thread hung")
    bad = [f"rank {r}: {e}" for r, e in enumerate(err) if e]
    if bad:
        raise AssertionError("; ".join(bad))
    return out


def rccl_world(P):
    uid = mpi.unique_id()

    def body(r):
        h = ctypes.c_void_p()
        _lib.call("mpjx_comm_init_rank", ctypes.byref(h), P, uid, r, 0)
        c = mpi.Intracomm(h.value)
        c._kind = "rccl"
        return c
    return threads(P, body)


def standin_calls(L):
    L.rsi_log.restype = ctypes.c_size_t
    L.rsi_log.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    n = L.rsi_log(None, 0)
    buf = ctypes.create_string_buffer(n)
    L.rsi_log(buf, n)
    calls = {}
    for e in json.loads(buf.value.decode()):
        k = e.get("op", "error")
        calls[k] = calls.get(k, 0) + 1
    return calls


def main():
    engine, Ps, tnames = sys.argv[1], [int(p) for p in sys.argv[2].split(",")], sys.argv[3].split(",")
    L = _lib.lib()
    if engine == "rccl":
        assert L.rsi_is_standin() == 1, "MPJX_LIB_PATH does not name the stand-in build"
    bad, n = [], 0
    try:
        for P in Ps:
            comms = rccl_world(P) if engine == "rccl" else mpi.smp_world(P, [0] * P)
            todo = [(coll, root, MC.make_case(coll, P, t, root)) for coll, p_, t, root in MC.matrix([P], tnames)]
            try:
                out = threads(P, lambda r: [MC.run_rank(torch, comms[r], coll, ranks[r], root)
                                            for coll, root, ranks in todo])
                bad += [m for res in out for m in res if m]
                n += len(todo)
            finally:
                threads(P, lambda r: comms[r].Free())
    except BaseException as e:  # noqa: BLE001
        bad.append(f"raised {e!r}"[:2000])
    calls = standin_calls(L) if engine == "rccl" else {}
    print(json.dumps({"cases": n, "bad": bad, "calls": calls}), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
