"""One rank process of an IPC world (mpjx_comm_init_ipc) running the strided block moves, started by
tests/test_gpu_strided_ipc.py.

    python tests/strided_ipc_worker.py RANK P UID_HEX BASE

Every rank builds the whole case (tests/strided_cases.py, seeded) and checks its own receive buffer, whole, and
its send buffer. IPC worlds take the pack -> IpcTransport::exchange -> unpack engine. Prints one JSON line:
{"rank": r, "cases": n, "bad": [messages]}.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]

import torch  # noqa: E402

import strided_cases as SC  # noqa: E402
from mpjexpress_amd import mpi  # noqa: E402


def main():
    rank, P, uid_hex, base = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    torch.cuda.set_device(0)
    comm = mpi.InitIPC(rank, P, 0, bytes.fromhex(uid_hex))
    todo, types, bad = SC.matrix(P), {}, []
    for case in todo:
        print(f"rank {rank} {case}", flush=True)
        bad += SC.run_methods(torch, comm, P, base, [case], types)
    for t in types.values():
        t.Free()
    comm.Free()
    print(json.dumps({"rank": rank, "cases": len(todo), "bad": bad}), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
