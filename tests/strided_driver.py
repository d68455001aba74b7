"""Runs the strided block moves' method matrix (tests/strided_cases.py) on rank threads in a fresh process.

    python tests/strided_driver.py smp|rccl P[,P...] BASE[,BASE...]

The worlds are tests/moves_driver.py's: `rccl` forms an "RCCL" world per P over the stand-in build the caller
names in MPJX_LIB_PATH (tests/test_gpu_strided_standin.py does), so the pack -> RcclTransport::exchange ->
unpack engine carries the moves; the stand-in's log of the RCCL calls libmpjx made is reported.
Prints one JSON line: {"cases": n, "bad": [messages], "calls": {rccl call: count}}.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]

import torch  # noqa: E402

import moves_driver as MD  # noqa: E402
import strided_cases as SC  # noqa: E402
from mpjexpress_amd import _lib, mpi  # noqa: E402


def rank_body(comm, P, base, todo):
    types = {}
    try:
        return SC.run_methods(torch, comm, P, base, todo, types)
    finally:
        for t in types.values():
            t.Free()


def main():
    engine, Ps, bases = sys.argv[1], [int(p) for p in sys.argv[2].split(",")], sys.argv[3].split(",")
    L = _lib.lib()
    if engine == "rccl":
        assert L.rsi_is_standin() == 1, "MPJX_LIB_PATH does not name the stand-in build"
    bad, n = [], 0
    try:
        for P in Ps:
            comms = MD.rccl_world(P) if engine == "rccl" else mpi.smp_world(P, [0] * P)
            todo = SC.matrix(P)
            try:
                for base in bases:
                    out = MD.threads(P, lambda r: rank_body(comms[r], P, base, todo))
                    bad += [m for res in out for m in res]
                    n += len(todo)
            finally:
                MD.threads(P, lambda r: comms[r].Free())
    except BaseException as e:  # noqa: BLE001
        bad.append(f"raised {e!r}"[:2000])
    calls = MD.standin_calls(L) if engine == "rccl" else {}
    print(json.dumps({"cases": n, "bad": bad, "calls": calls}), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
