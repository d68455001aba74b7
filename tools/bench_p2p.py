"""Point-to-point timing: a ping-pong between two rank threads (8 B .. 1 MiB) and the P = 4 halo exchange of
tests/test_gpu_p2p_halo.py on 1024 x 1024 DOUBLE tiles, each timed three ways:

  batched     the default: a wait moves every matched message in one k_msgs launch
  families    MPJX_P2P_BATCH=0: one launch per kernel family (DtMoves::launch)
  alltoallv   torch pack + the existing Alltoallv of the same bytes: what a caller could do before these calls

  python tools/bench_p2p.py [--iters 30] [--warmup 5] [--sizes 8,1024,...] [--tile 1024] [--out FILE]

Times are host wall-clock per BLOCKING exchange (the calls return complete), the median over --iters, on cold
operands: before every timed exchange rank 0 rewrites a 512 MiB scratch buffer, twice the 256 MiB Infinity
Cache the ranks share, outside the timed region, and the ranks meet at a barrier. A ping-pong row is half a round trip. One JSON
line per row."""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mpjexpress_amd import mpi  # noqa: E402
from mpjexpress_amd.mpi import MPI, Datatype, Request  # noqa: E402

FLUSH_BYTES = 512 << 20


def run(comms, fn):
    out, err = [None] * len(comms), [None] * len(comms)

    def body(r):
        try:
            torch.cuda.set_device(0)
            out[r] = fn(comms[r])
        except BaseException as e:  # noqa: BLE001
            err[r] = e
    ts = [threading.Thread(target=body, args=(r,)) for r in range(len(comms))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for e in err:
        if e is not None:
            raise e
    return out


def world(P, batch):
    old = os.environ.pop("MPJX_P2P_BATCH", None)
    if not batch:
        os.environ["MPJX_P2P_BATCH"] = "0"
    try:
        comms = mpi.smp_world(P, [0] * P)
    finally:
        os.environ.pop("MPJX_P2P_BATCH", None)
        if old is not None:
            os.environ["MPJX_P2P_BATCH"] = old
    return comms


def timed(c, flush, step, iters, warmup):
    """Median seconds of step() over iters cold runs (rank 0's clock; every rank runs step)."""
    ts = []
    for i in range(warmup + iters):
        if c.Rank() == 0:
            flush.add_(1)  # one rank evicts the shared cache; the others wait at the barrier
            torch.cuda.synchronize()
        c.Barrier()
        t0 = time.perf_counter()
        step()
        t1 = time.perf_counter()
        if i >= warmup:
            ts.append(t1 - t0)
    return statistics.median(ts)


def pingpong(a, mode, flush):
    comms = world(2, mode != "families")
    rows = []

    def body(c):
        me, other, res = c.Rank(), 1 - c.Rank(), []
        for nbytes in a.sizes:
            n = nbytes // 8
            s = torch.arange(n, dtype=torch.float64, device="cuda")
            r = torch.zeros(n, dtype=torch.float64, device="cuda")
            z, to1, to0 = [0, 0], [0, n], [n, 0]

            def step():
                if mode == "alltoallv":  # 0 -> 1, then 1 -> 0
                    c.Alltoallv(s, 0, to1 if me == 0 else z, z, MPI.DOUBLE, r, 0, z if me == 0 else to0, z, MPI.DOUBLE)
                    c.Alltoallv(s, 0, z if me == 0 else to0, z, MPI.DOUBLE, r, 0, to1 if me == 0 else z, z, MPI.DOUBLE)
                elif me == 0:
                    c.Send(s, 0, n, MPI.DOUBLE, other, 0)
                    c.Recv(r, 0, n, MPI.DOUBLE, other, 0)
                else:
                    c.Recv(r, 0, n, MPI.DOUBLE, other, 0)
                    c.Send(s, 0, n, MPI.DOUBLE, other, 0)
            t = timed(c, flush, step, a.iters, a.warmup)
            res.append({"bench": "pingpong", "mode": mode, "bytes": nbytes, "us_one_way": round(t * 1e6 / 2, 2)})
        return res
    rows = run(comms, body)[0]
    for c in comms:
        c.Free()
    return rows


def halo(a, mode, flush):
    comms = world(4, mode != "families")
    T = a.tile
    N = T + 2
    col = Datatype.Vector(T, 1, N, MPI.DOUBLE)

    def body(c):
        me = c.Rank()
        i, j = divmod(me, 2)
        nb = {"n": ((i - 1) % 2) * 2 + j, "s": ((i + 1) % 2) * 2 + j, "w": i * 2 + (j - 1) % 2, "e": i * 2 + (j + 1) % 2}
        t = (torch.arange(N * N, dtype=torch.float64, device="cuda") + me * 1e7)
        t2 = t.view(N, N)
        sbuf = torch.zeros(4 * 2 * T, dtype=torch.float64, device="cuda")
        rbuf = torch.zeros(4 * 2 * T, dtype=torch.float64, device="cuda")
        at = lambda r, k: r * N + k  # noqa: E731

        def step():
            if mode == "alltoallv":
                # periodic 2 x 2: north = south and west = east, so two peers get two messages each and the
                # diagonal rank none; slot k of peer p at (2 p + k) T
                order = (("n", t2[1, 1:N - 1], 0), ("s", t2[N - 2, 1:N - 1], 1), ("w", t2[1:N - 1, 1], 0), ("e", t2[1:N - 1, N - 2], 1))
                for d, src, k in order:
                    sbuf[(2 * nb[d] + k) * T:(2 * nb[d] + k + 1) * T] = src
                cnt = [2 * T if p in (nb["n"], nb["w"]) else 0 for p in range(4)]
                dis = [2 * T * p for p in range(4)]
                c.Alltoallv(sbuf, 0, cnt, dis, MPI.DOUBLE, rbuf, 0, cnt, dis, MPI.DOUBLE)
                t2[N - 1, 1:N - 1] = rbuf[(2 * nb["s"] + 0) * T:(2 * nb["s"] + 1) * T]
                t2[0, 1:N - 1] = rbuf[(2 * nb["n"] + 1) * T:(2 * nb["n"] + 2) * T]
                t2[1:N - 1, N - 1] = rbuf[(2 * nb["e"] + 0) * T:(2 * nb["e"] + 1) * T]
                t2[1:N - 1, 0] = rbuf[(2 * nb["w"] + 1) * T:(2 * nb["w"] + 2) * T]
                torch.cuda.synchronize()
                return
            req = [
                c.Irecv(t, at(N - 1, 1), T, MPI.DOUBLE, nb["s"], 0), c.Irecv(t, at(0, 1), T, MPI.DOUBLE, nb["n"], 1),
                c.Irecv(t, at(1, N - 1), 1, col, nb["e"], 2), c.Irecv(t, at(1, 0), 1, col, nb["w"], 3),
                c.Isend(t, at(1, 1), T, MPI.DOUBLE, nb["n"], 0), c.Isend(t, at(N - 2, 1), T, MPI.DOUBLE, nb["s"], 1),
                c.Isend(t, at(1, 1), 1, col, nb["w"], 2), c.Isend(t, at(1, N - 2), 1, col, nb["e"], 3),
            ]
            Request.Waitall(req)
        sec = timed(c, flush, step, a.iters, a.warmup)
        return {"bench": "halo", "mode": mode, "tile": T, "bytes_per_rank": 4 * T * 8, "us": round(sec * 1e6, 2),
                "stats": c.p2p_stats()}
    rows = run(comms, body)
    col.Free()
    for c in comms:
        c.Free()
    out = rows[0]
    out["launches_all_ranks"] = sum(r["stats"][0] for r in rows)
    out.pop("stats")
    return [out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="8,64,512,4096,32768,131072,262144,1048576")
    ap.add_argument("--tile", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.sizes = [int(x) for x in a.sizes.split(",")]
    torch.cuda.set_device(0)
    flush = torch.zeros(FLUSH_BYTES // 4, dtype=torch.int32, device="cuda")
    rows = []
    for mode in ("batched", "families", "alltoallv"):
        rows += pingpong(a, mode, flush)
        rows += halo(a, mode, flush)
    text = "\n".join(json.dumps(r) for r in rows)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
