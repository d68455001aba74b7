"""Runs tests/struct_cases.py on rank threads in a fresh process.

    python tests/struct_driver.py smp|rccl P[,P...]

The worlds are tests/moves_driver.py's: `rccl` forms an "RCCL" world per P over the stand-in build the caller names
in MPJX_LIB_PATH (tests/test_gpu_struct.py does), so the exchange engines' pack and unpack launches carry the
Struct and resized types, the element transposes among them.
Prints one JSON line: {"cases": n, "bad": [messages], "kernels": [OR of every rank's masks after the transposing
Alltoall], "calls": {rccl call: count}}.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]

import torch  # noqa: E402

import moves_driver as MD  # noqa: E402
import struct_cases as ST  # noqa: E402
from mpjexpress_amd import _lib, mpi  # noqa: E402


def rank_body(comm, P):
    bad = ST.alltoall_transpose(torch, comm, P)
    m = ctypes.c_uint()
    _lib.call("mpjx_comm_last_move_kernels", comm.handle, ctypes.byref(m))
    for fn in ST.FAMILIES[1:]:
        bad += fn(torch, comm, P)
    return bad, m.value


def main():
    engine, Ps = sys.argv[1], [int(p) for p in sys.argv[2].split(",")]
    L = _lib.lib()
    if engine == "rccl":
        assert L.rsi_is_standin() == 1, "MPJX_LIB_PATH does not name the stand-in build"
    bad, n, kernels = [], 0, []
    try:
        for P in Ps:
            comms = MD.rccl_world(P) if engine == "rccl" else mpi.smp_world(P, [0] * P)
            try:
                out = MD.threads(P, lambda r: rank_body(comms[r], P))
                bad += [m for res in out for m in res[0]]
                kernels.append([res[1] for res in out])
                n += len(ST.FAMILIES)
            finally:
                MD.threads(P, lambda r: comms[r].Free())
    except BaseException as e:  # noqa: BLE001
        bad.append(f"raised {e!r}"[:2000])
    calls = MD.standin_calls(L) if engine == "rccl" else {}
    print(json.dumps({"cases": n, "bad": bad, "kernels": kernels, "calls": calls}), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
