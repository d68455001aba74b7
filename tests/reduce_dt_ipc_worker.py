"""One rank process of an IPC world (mpjx_comm_init_ipc) running the reductions on derived datatypes, started by
tests/test_gpu_reduce_dt_ipc.py.

    python tests/reduce_dt_ipc_worker.py RANK P UID_HEX

Every rank builds the whole seeded world (tests/reduce_dt_cases.py's child_cases) and checks its own receive
buffer, whole, and its send buffer. An IPC world's ranks sit in different processes, so every call takes the pack
path: pack -> the contiguous call on the IPC engine -> unpack. Prints one JSON line:
{"rank": r, "cases": n, "bad": [messages]}.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), HERE]

import torch  # noqa: E402

import reduce_dt_cases as RC  # noqa: E402
from mpjexpress_amd import mpi  # noqa: E402


def main():
    rank, P, uid_hex = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    torch.cuda.set_device(0)
    comm = mpi.InitIPC(rank, P, 0, bytes.fromhex(uid_hex))
    cases = RC.child_cases(P)
    try:
        bad = RC.run_cases(torch, comm, cases, RC.FORM_PACK)
    finally:
        comm.Free()
    print(json.dumps({"rank": rank, "cases": len(cases), "bad": bad}), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
