"""One rank process of an IPC world (mpjx_comm_init_ipc) running the block-move collectives, started by
tests/test_gpu_moves_ipc.py.

    python tests/moves_ipc_worker.py RANK P UID_HEX TYPE[,TYPE...]

Every rank builds the whole case (tests/moves_cases.py, seeded) and checks its own receive buffer, whole,
and its send buffer. IPC worlds take the exchange path: the rank's own block by k_moves, the rest through
IpcTransport::exchange. Prints one JSON line: {"rank": r, "cases": n, "bad": [messages]}.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]

import torch  # noqa: E402

import moves_cases as MC  # noqa: E402
from mpjexpress_amd import mpi  # noqa: E402


def main():
    rank, P, uid_hex, tnames = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4].split(",")
    torch.cuda.set_device(0)
    comm = mpi.InitIPC(rank, P, 0, bytes.fromhex(uid_hex))
    bad, n = [], 0
    # torch's caching allocator hands no device memory back while the world lives
    for coll, p_, tname, root in MC.matrix([P], tnames):
        print(f"rank {rank} {coll} {tname} root {root}", flush=True)
        ranks = MC.make_case(coll, P, tname, root)
        msg = MC.run_rank(torch, comm, coll, ranks[rank], root)
        if msg:
            bad.append(msg)
        n += 1
    comm.Free()
    print(json.dumps({"rank": rank, "cases": n, "bad": bad}), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
